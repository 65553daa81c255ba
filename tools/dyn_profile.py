"""Estimated DYNAMIC instruction profile of a kernel by source line: static ISA count per line (hipcc -S -g) x execution
count per line from a gcov run of the host emulation (tests/emu built with --coverage).  Lines inside the emulated-lane
loops of parse_core.h (PC_VEC_BEGIN..PC_VEC_END) run 64x per wave step on the host and are scaled back.  Dev tool.
usage: dyn_profile.py <kernel.hip> <kernel-symbol-substring> <source-with-gcov> <file.gcov> [pixels]
env: SALU=1 / VS=1 / SPILL=1 add the top lines of that class, BY_ELEMENT=1 the parser's table by syntax element, TOPN=<lines>,
SKIP_LINES=<a-b,c,...> source lines left out of every total (a spin wait whose count is the host's thread scheduling, not the kernel's work)"""
import collections, os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
kern, sym, srcname, gcovf = sys.argv[1:5]
px = float(sys.argv[5]) if len(sys.argv) > 5 else None
out = "/tmp/isa_%s.s" % os.path.basename(kern)
subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-g", "-std=c++17", "-ffp-contract=off", "-I%s/include" % ROOT,
                       "-I%s/libheif_amd/csrc" % ROOT, "-S", "--cuda-device-only", "-o", out, kern] + os.environ.get("EXTRA", "").split(), stderr=subprocess.DEVNULL)
lines = open(out).read().split("\n")
start = [i for i, l in enumerate(lines) if re.match(r"^_Z\S*%s\S*:" % re.escape(sym), l)][0]
files = {}
for l in lines:
    m = re.match(r'\s+\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m: files[int(m.group(1))] = (m.group(3) or m.group(2))
static = collections.Counter(); static_cls = collections.Counter(); cur = None
for l in lines[start:]:
    m = re.match(r"\s+\.loc\s+(\d+)\s+(\d+)", l)
    if m: cur = (files.get(int(m.group(1)), ""), int(m.group(2))); continue
    if l.startswith(".Lfunc_end"): break
    if re.match(r"\s+[a-z_0-9]+(\s|$)", l) and not l.strip().startswith((".", ";")):
        static[cur] += 1
        op = l.split()[0]
        cls = "B" if op.startswith(("s_cbranch", "s_branch")) else ("N" if op.startswith(("s_nop", "s_waitcnt")) else ("S" if op.startswith("s_") else ("V" if op.startswith("v_") else "M")))
        # round 6 (profiles/r06_issue_model_*.txt): a VALU instruction that reads or writes the scalar register file (SGPR operand, VCC, v_readlane,
        # v_cmp, v_cndmask ...) issues at half the rate of one that only touches VGPRs / inline constants: class "Vs" against "Vp"
        if cls == "V":
            args = l.split(";")[0].split(None, 1)[1] if len(l.split(";")[0].split(None, 1)) > 1 else ""
            sg = bool(re.search(r"(?<![a-z0-9_])(s\d+|s\[\d+:\d+\]|vcc|vcc_lo|vcc_hi|exec|m0|scc)(?![a-z0-9_])", args)) or op.startswith(("v_cmp", "v_readlane", "v_readfirstlane", "v_writelane"))
            static_cls[(cur, "Vs" if sg else "Vp")] += 1
            # SGPR spills live in VGPR lanes: a reload is v_readlane sN, vK, <constant lane>, a spill v_writelane vK, sN, <constant lane>
            if re.match(r"v_readlane_b32\s+s\d+,\s*v\d+,\s*\d+\s*$", l.split(";")[0].strip()): static_cls[(cur, "spill_reload")] += 1
            if re.match(r"v_writelane_b32\s+v\d+,\s*s\d+,\s*\d+\s*$", l.split(";")[0].strip()): static_cls[(cur, "spill_store")] += 1
        static_cls[(cur, cls)] += 1
st_line = collections.Counter()
unattributed = 0
for (f, ln), c in static.items():
    if f.endswith(srcname) and ln: st_line[ln] += c
    else: unattributed += c
print("static instructions: %d in %s, %d elsewhere / line 0" % (sum(st_line.values()), srcname, unattributed))
# gcov
dyn = {}
text = {}
for l in open(gcovf):
    m = re.match(r"\s*([0-9#=\-\*]+)\*?:\s*(\d+):(.*)", l)
    if not m: continue
    ln = int(m.group(2)); text[ln] = m.group(3)
    c = m.group(1)
    if c.rstrip("*").isdigit(): dyn[ln] = int(c.rstrip("*"))
# vector regions
invec = set(); on = False
for ln in sorted(text):
    t = text[ln]
    if "PC_VEC_BEGIN" in t and "define" not in t: on = True
    if on: invec.add(ln)
    if "PC_VEC_END" in t and "define" not in t: on = False
skip = set()
for part in filter(None, os.environ.get("SKIP_LINES", "").split(",")):
    lo, _, hi = part.partition("-")
    skip.update(range(int(lo), int(hi or lo) + 1))
def count(ln):
    if ln in skip: return 0
    # nearest executed line at or before ln (declarations / continuation lines carry no count)
    for k in range(ln, max(ln - 6, 0), -1):
        if k in dyn:
            c = dyn[k]
            return c / 64.0 if k in invec else c   # the emulated-lane loop runs its header 65x and its body 64x per wave step
    return 0
# enclosing function of every line (heuristic) and the number of inlined copies of each function: every copy
# contributes at least one instruction to each executed statement, so the smallest static count of a function's
# lines estimates the number of copies; static counts are divided by it before weighting with the execution counts
func_at = {}; curf = "?"
for ln in sorted(text):
    t = text[ln]
    m = re.match(r"(?:PC_DEV|__device__|static|template|inline)\b.*?\b([a-z_0-9]+)\s*\(", t)
    if m and not t.startswith(" "): curf = m.group(1)
    func_at[ln] = curf
copies = {}
for ln, c in st_line.items():
    if count(ln) > 0:
        f = func_at.get(ln, "?"); copies[f] = min(copies.get(f, 1 << 30), c)
tot = 0; rows = []
cls_tot = collections.Counter()
for ln, c in st_line.items():
    k = max(1, copies.get(func_at.get(ln, "?"), 1))
    d = c / k * count(ln); tot += d; rows.append((d, ln, c / k, count(ln)))
    for (key, cls), cc in static_cls.items():
        if key[1] == ln and key[0].endswith(srcname): cls_tot[cls] += cc / k * count(ln)
print("by class (S salu, V valu = Vs scalar-file-touching + Vp pure, B branch, N nop/waitcnt, M memory/lds):", {k: round(v / (px or 1), 2) for k, v in cls_tot.items()})
srows = []
for (key, cls), cc in static_cls.items():
    if cls == "S" and key[0].endswith(srcname) and key[1]:
        ln = key[1]; k = max(1, copies.get(func_at.get(ln, "?"), 1))
        srows.append((cc / k * count(ln), ln, cc / k, count(ln)))
srows.sort(reverse=True)
if os.environ.get("SPILL"):
    for what in ("spill_reload", "spill_store"):
        vrows = []
        for (key, cls), cc in static_cls.items():
            if cls == what and key[0].endswith(srcname) and key[1]:
                ln = key[1]; k = max(1, copies.get(func_at.get(ln, "?"), 1))
                vrows.append((cc / k * count(ln), ln, cc / k, count(ln)))
        vrows.sort(reverse=True)
        print("-- %s: %.2f per pixel; top lines" % (what, sum(r[0] for r in vrows) / (px or 1)))
        for d, ln, c, k in vrows[:int(os.environ.get("TOPN", "45"))]: print("%5.2f/px line %4d static %5.1f x %9.0f  %s" % (d / (px or 1), ln, c, k, text[ln].strip()[:100]))
if os.environ.get("VS"):
    vrows = []
    for (key, cls), cc in static_cls.items():
        if cls == "Vs" and key[0].endswith(srcname) and key[1]:
            ln = key[1]; k = max(1, copies.get(func_at.get(ln, "?"), 1))
            vrows.append((cc / k * count(ln), ln, cc / k, count(ln)))
    vrows.sort(reverse=True)
    vbyf = collections.Counter()
    for d, ln, c, k in vrows: vbyf[func_at.get(ln, "?")] += d
    print("-- scalar-file-touching VALU by function:", {f: round(d / (px or 1), 2) for f, d in vbyf.most_common(14)})
    print("-- top scalar-file-touching VALU lines")
    for d, ln, c, k in vrows[:int(os.environ.get("TOPN", "45"))]: print("%5.2f/px line %4d static %5.1f x %9.0f  %s" % (d / (px or 1), ln, c, k, text[ln].strip()[:100]))
if os.environ.get("SALU"):
    sbyf = collections.Counter()
    for d, ln, c, k in srows: sbyf[func_at.get(ln, "?")] += d
    print("-- SALU by function:", {f: round(d / (px or 1), 2) for f, d in sbyf.most_common(12)})
    print("-- top SALU lines")
    for d, ln, c, k in srows[:int(os.environ.get("TOPN", "45"))]: print("%5.2f/px line %4d static %5.1f x %9.0f  %s" % (d / (px or 1), ln, c, k, text[ln].strip()[:100]))
if os.environ.get("BY_ELEMENT"):
    # the parser's estimate by SYNTAX ELEMENT (profiles/parse_residual_glue.txt): a group starts at the first line of its function that matches the
    # anchor and runs to the next anchor or the function's end; a function without anchors is one group.  Occurrences: executions of the anchor line.
    # SGPR spill reloads / stores (v_readlane / v_writelane with a constant lane) are taken out of their groups and shown as a class of their own.
    ANCHORS = [("residual_coding", r"^PC_DEV int residual_coding", "transform_skip, last_x / last_y prefix and suffix"),
               ("residual_coding", r"int scan_idx = 0;", "last-position lookup"),
               ("residual_coding", r"uint64_t csbf = 0;", "sub-block loop control and csbf"),
               ("residual_coding", r"per-sub-block sig_coeff_flag context selection|const uint32_t pat = log2n == 2|const uint32_t sig_row = ", "sig-context setup"),
               ("residual_coding", r"^#else", "sub-block loop control and csbf"),
               ("residual_coding", r"sig_coeff_flag contexts of the 16 scan positions", "sig-context setup"),
               ("residual_coding", r"// greater1 / greater2 flags", "greater1 / greater2 glue"),
               ("residual_coding", r"// coeff_sign_flag:", "sign and remaining glue"),
               ("residual_coding", r"// levels, signs \(incl", "level assembly and store"),
               ("residual_coding", r"VReg vbad;", "overflow check"),
               ("coding_unit", r"^PC_DEV void coding_unit", "coding_unit"),
               ("coding_unit", r"// ---- transform tree ----", "transform-tree glue (cbf, split, destination, map arguments)")]
    FUNCS = {"scan_sb": "sub-block loop control and csbf", "zero_uncoded_sub_blocks": "level assembly and store",
             "pc_lds_u16": "sig-context setup", "tu_sig_row": "sig-context setup", "pc_lds_u8": "sub-block loop control and csbf",
             "tu_scan_idx": "last-position lookup",
             "load_tu_tables": "CTB loop, quadtree, SAO, publish",
             "win_byte": "byte reading", "win_prime": "byte reading", "win_advance": "byte reading",
             "fill_tu_maps": "transform-tree glue (cbf, split, destination, map arguments)", "parse_cu_qp_delta": "coding_unit", "derive_qp_pred": "coding_unit",
             "set_qp_y": "coding_unit", "left_cb_log2": "coding_unit", "up_cb_log2": "coding_unit",
             "read_byte_v": "byte reading", "read_byte": "byte reading", "refill_byte": "byte reading", "load_window": "byte reading", "fetch_byte": "byte reading",
             "map_fill": "unit-map access (map_fill, map_get, interleave4)", "map_get": "unit-map access (map_fill, map_get, interleave4)",
             "map_get2": "unit-map access (map_fill, map_get, interleave4)", "interleave4": "unit-map access (map_fill, map_get, interleave4)",
             "compact1by1": "unit-map access (map_fill, map_get, interleave4)",
             "decode_remaining_v": "decode helpers (bypass, remaining: not glue)", "decode_remaining": "decode helpers (bypass, remaining: not glue)",
             "decode_bypass_multi": "decode helpers (bypass, remaining: not glue)", "decode_bypass_bits": "decode helpers (bypass, remaining: not glue)",
             "decode_bypass": "decode helpers (bypass, remaining: not glue)", "parse_substream": "CTB loop, quadtree, SAO, publish", "parse_sao": "CTB loop, quadtree, SAO, publish"}
    group_at = {}; occ_line = {}; curg = None; lastf = None
    for ln in sorted(text):
        f = func_at.get(ln, "?")
        if f != lastf: curg = FUNCS.get(f, "everything else"); lastf = f
        for af, rx, g in ANCHORS:
            if af == f and re.search(rx, text[ln]):
                # the #else anchor only counts inside the sub-block loop's two forms of the head
                if rx == r"^#else" and curg != "sig-context setup": continue
                curg = g
                if g not in occ_line: occ_line[g] = ln
        group_at[ln] = curg
    def occurrences(g):
        ln = occ_line.get(g)
        if ln is None: return 0
        for k in range(ln, ln + 12):
            if k in dyn and dyn[k] > 0 and group_at.get(k) == g: return dyn[k] / 64.0 if k in invec else dyn[k]
        return 0
    gt = collections.defaultdict(collections.Counter)
    for (key, cls), cc in static_cls.items():
        if not (key[0].endswith(srcname) and key[1]): continue
        ln = key[1]; k = max(1, copies.get(func_at.get(ln, "?"), 1))
        gt[group_at.get(ln, "everything else")][cls] += cc / k * count(ln)
    print("-- by syntax element: instructions per pixel without SGPR spill traffic | per occurrence | scalar-file-touching (SALU + branch + Vs) | pure VALU | other (nop / waitcnt / memory)")
    order = []
    for _, _, g in ANCHORS:
        if g not in order: order.append(g)
    for g in FUNCS.values():
        if g not in order: order.append(g)
    order.append("everything else")
    sp_r = sp_s = 0.0; tsum = 0.0
    for g in order:
        c = gt.get(g)
        if not c: continue
        spill = c["spill_reload"] + c["spill_store"]; sp_r += c["spill_reload"]; sp_s += c["spill_store"]
        scal = c["S"] + c["B"] + c["Vs"] - spill; pure = c["Vp"]; other = c["N"] + c["M"]
        tot_g = scal + pure + other; tsum += tot_g
        o = occurrences(g)
        print("%-62s %6.2f  %8s  %6.2f  %6.2f  %6.2f" % (g, tot_g / (px or 1), ("%.1f" % (tot_g / o)) if o else "-", scal / (px or 1), pure / (px or 1), other / (px or 1)))
    print("%-62s %6.2f  (reloads %.2f, stores %.2f)" % ("SGPR spill reloads and stores", (sp_r + sp_s) / (px or 1), sp_r / (px or 1), sp_s / (px or 1)))
    print("%-62s %6.2f" % ("sum", (tsum + sp_r + sp_s) / (px or 1)))
rows.sort(reverse=True)
print("estimated dynamic wave-instructions: %.3g%s" % (tot, (" = %.1f per pixel" % (tot / px)) if px else ""))
byf = collections.Counter()
for d, ln, c, k in rows: byf[func_at.get(ln, "?")] += d
print("-- by function")
for f, d in byf.most_common(25): print("%6.2f%%  %s" % (100 * d / tot, f))
print("-- top lines")
for d, ln, c, k in rows[:int(os.environ.get("TOPN", "45"))]: print("%5.2f%% line %4d static %5.1f x %9.0f  %s" % (100 * d / tot, ln, c, k, text[ln].strip()[:100]))
