"""Composed tensor output against the way a host has without it, on one batch of 64 generator 4K stills (8-bit 4:2:0), all in one process on the same build,
interleaved rounds: YOLO's mosaic-4 - 256 entries (every still four times, two of them flipped), each resized to 640 x 360, four around a random centre on
each of 64 canvases of 1280 x 1280, float16 NCHW, grey 114 elsewhere; the centres are drawn with a fixed seed from the middle half of the canvas.  BILINEAR
decides; BOX and BICUBIC are reported beside it without a bar.
Two ways, both into torch tensors on one torch stream, timed by a pair of events on that stream around everything a way enqueues.  A few milliseconds of
other work are put on the stream in front of the first event, so that a way's launches are queued before the device reaches them: the time between the events
is the device's, not the host's preparation of the calls:
 composed   ONE to_tensor_composed(tiles=mosaic_tiles(...)) call: one k_frame_* launch over the 256 pieces, one k_compose_cover launch over the 64 canvases;
 two-step   to_tensor at 640 x 360 into a scratch tensor, one torch fill of the canvases with the grey element, then 256 clipped slice copies.
Expectation, written into the report BEFORE the run: one composed call is not slower than the two-step way.  The bar is the two-step way's mean plus its own
max - min spread over the rounds; HELD or REFUTED is reported with both figures; the results are compared bit for bit.
The cover kernel by difference: the same composed call with a whole-canvas base entry under each mosaic has no unowned pixel and launches no cover kernel;
its base pieces are picture work over the pixels the cover kernel fills, so (composed - based) is the cover launch MINUS that work: positive, it bounds the
cover launch's time from below and its rate from above; negative or inside the spread, no rate follows and the report says so.  Beside it, from the same run,
k_canvas_margin by the same method: a placed call whose margins hold the same number of bytes against the placed call with whole-canvas rectangles.
Where neither difference gives a rate, the direct pair does: a composed call whose four entries per canvas are 8 x 8 samples of 16 x 16 windows around the
mosaic's centre, and a placed call with one 16 x 16 rectangle there - almost no picture work, so the call's time over the fill bytes is a lower bound of the
rate of k_compose_cover and of k_canvas_margin over nearly the whole tensor.  The kernels' VGPR counts are read from the code object and reported beside it.
usage: python tools/measure_composed_output.py [report.txt] [--rehearse], from the repository root after build(); --rehearse runs two small stills once through
every call (no 4K streams needed, the numbers mean nothing)."""
import glob, os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
import libheif_amd
from libheif_amd import decoder

args = [a for a in sys.argv[1:] if not a.startswith("--")]
REHEARSE = "--rehearse" in sys.argv
out = open(args[0] if args else os.devnull, "w")
def say(s):
    print(s); out.write(s + "\n"); out.flush()

import torch
if not torch.cuda.is_available():
    say("not measured: torch sees no GPU (the two-step way is made of torch calls)")
    sys.exit(1)

if REHEARSE:
    from oracle import pyoracle as orc
    W, H, N, SW, SH, CANVAS, R = 200, 136, 2, 40, 24, 64, 1
    streams = [orc.encode(orc.synth_image(W, H, 8, 1, seed=3 + i), bit_depth=8) for i in range(N)]
else:
    W, H, N, SW, SH, CANVAS, R = 3840, 2160, 64, 640, 360, 1280, 12
    files = sorted(glob.glob("build/streams/s_3840x2160_*.hevc"))[:N]
    assert len(files) == N, len(files)
    streams = [open(f, "rb").read() for f in files]
lib = decoder._bind(libheif_amd.load_library())
assert lib.hipdec_init(0) == 0
b = decoder.Batch(streams)
d = b.info(0)
assert (d["width"], d["height"], d["bit_depth_luma"], d["chroma_format_idc"]) == (W, H, 8, 1), d
b.run(); b.status()
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    ballast = torch.empty(64 << 20 if REHEARSE else 512 << 20, dtype=torch.uint8, device="cuda")

def timed(call):
    """device ms between two events on `side` around what `call` enqueues"""
    with torch.cuda.stream(side):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(8):
            ballast.zero_()                                          # the device is busy while the host prepares and enqueues the calls
        e0.record(side); call(); e1.record(side)
    side.synchronize(); b.status()
    return e0.elapsed_time(e1)

NC = N
n = 4 * NC
entries = [(i % N, 0, 0, 0, 0, (i // N) & 1) for i in range(n)]
rng = np.random.default_rng(2026)
centres = [(int(rng.integers(CANVAS // 4, 3 * CANVAS // 4)), int(rng.integers(CANVAS // 4, 3 * CANVAS // 4))) for _ in range(NC)]
tiles = []
for c, centre in enumerate(centres):
    tiles += decoder.mosaic_tiles((CANVAS, CANVAS), centre, [(SW, SH)] * 4, c)
area = decoder.compose_visible_area((CANVAS, CANVAS), tiles, NC)
unowned = NC * CANVAS * CANVAS - sum(area)
# the same call with a whole-canvas base entry under each mosaic: every pixel is owned, no cover launch
based_entries = [(c % N, 0, 0, 0, 0, 0) for c in range(NC)] + entries
based_tiles = [(c, (0, 0, CANVAS, CANVAS), (0, 0, 0, 0)) for c in range(NC)] + tiles
# a placed call with the same number of margin pixels per canvas: one rectangle of the canvas' width
rows = max(1, min(CANVAS - 1, round((NC * CANVAS * CANVAS - unowned) / NC / CANVAS)))
places = [(0, 0, CANVAS, rows)] * NC
placed_entries = [(c % N, 0, 0, 0, 0, 0) for c in range(NC)]

# the direct pair: almost no picture work, the fill over nearly the whole tensor
tiny_entries = [(i % N, 0, 0, 16, 16, 0) for i in range(n)]
tiny_tiles = [(c, (xc - 8 + 8 * (k & 1), yc - 8 + 8 * (k >> 1), 8, 8), (0, 0, 0, 0)) for c, (xc, yc) in enumerate(centres) for k in range(4)]
tiny_places = [(xc - 8, yc - 8, 16, 16) for xc, yc in centres]
tiny_bytes = 3 * 2 * (NC * CANVAS * CANVAS - NC * 256)

def regions():
    for e, (cv, (x, y, w, h), (cx, cy, cw, ch)) in enumerate(tiles):
        x0, y0, x1, y1 = max(x, cx, 0), max(y, cy, 0), min(x + w, cx + cw, CANVAS), min(y + h, cy + ch, CANVAS)
        yield e, cv, x0, y0, x1, y1, x, y
REGIONS = list(regions())

def mean_spread(t):
    t = np.array(t)
    return t.mean(), t.max() - t.min(), t

def shape(fname, filt, bar):
    kw = dict(dtype="float16", layout="NCHW", mean=MEAN, std=STD, filter=filt)
    with torch.cuda.stream(side):
        composed = torch.empty((NC, 3, CANVAS, CANVAS), dtype=torch.float16, device="cuda")
        other = torch.empty((NC, 3, CANVAS, CANVAS), dtype=torch.float16, device="cuda")
        based = torch.empty((NC, 3, CANVAS, CANVAS), dtype=torch.float16, device="cuda")
        scratch = torch.empty((n, 3, SH, SW), dtype=torch.float16, device="cuda")
        sc, bi = decoder.tensor_scale_bias(MEAN, STD, None, None, 255)
        grey = torch.tensor((np.float32(114) * np.asarray(sc, np.float32) + np.asarray(bi, np.float32)).astype(np.float16), device="cuda").view(1, 3, 1, 1)
    def one_call():
        b.to_tensor_composed((CANVAS, CANVAS), tiles, entries, n_canvases=NC, fill=114, out=composed, **kw)
    def two_step():
        b.to_tensor((SW, SH), entries, out=scratch, **kw)
        other.copy_(grey.expand_as(other))
        for e, cv, x0, y0, x1, y1, x, y in REGIONS:
            other[cv, :, y0:y1, x0:x1] = scratch[e, :, y0 - y:y1 - y, x0 - x:x1 - x]
    def with_base():
        b.to_tensor_composed((CANVAS, CANVAS), based_tiles, based_entries, n_canvases=NC, fill=114, out=based, **kw)
    def placed():
        b.to_tensor((CANVAS, CANVAS), placed_entries, places=places, fill=114, out=based, **kw)
    def placed_whole():
        b.to_tensor((CANVAS, CANVAS), placed_entries, places=[(0, 0, CANVAS, CANVAS)] * NC, fill=114, out=based, **kw)
    def cover_only():
        b.to_tensor_composed((CANVAS, CANVAS), tiny_tiles, tiny_entries, n_canvases=NC, fill=114, out=based, **kw)
    def margin_only():
        b.to_tensor((CANVAS, CANVAS), [(c % N, 0, 0, 16, 16, 0) for c in range(NC)], places=tiny_places, fill=114, out=based, **kw)
    ways = [one_call, two_step] + ([with_base, placed, placed_whole, cover_only, margin_only] if bar else [])
    for c in ways:
        for _ in range(1 if REHEARSE else 2):
            timed(c)
    t = {c.__name__: [] for c in ways}
    for r in range(R):
        for c in (ways if r % 2 == 0 else ways[::-1]):
            t[c.__name__].append(timed(c))
    s0 = decoder.composed_stats()
    with torch.cuda.stream(side):
        one_call()
        s1 = decoder.composed_stats()
        two_step()
    side.synchronize(); b.status()
    same = bool(torch.equal(composed, other))
    m1, s1_, t1 = mean_spread(t["one_call"])
    m2, s2_, t2 = mean_spread(t["two_step"])
    say("")
    say("%s: %d entries at %d x %d on %d canvases of %d x %d, float16 NCHW; %d of %d pixels are unowned (%.0f %%)" %
        (fname, n, SW, SH, NC, CANVAS, CANVAS, unowned, NC * CANVAS * CANVAS, 100.0 * unowned / (NC * CANVAS * CANVAS)))
    say("  composed, one call                          events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f" % (m1, np.median(t1), t1.min(), t1.max()))
    say("  two-step: to_tensor + fill + %3d slice copies events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f" % (n, m2, np.median(t2), t2.min(), t2.max()))
    say("  per composed call: %d pieces, %d cover launch(es)" % ((s1[2] - s0[2]) // max(s1[0] - s0[0], 1), (s1[4] - s0[4]) // max(s1[0] - s0[0], 1)))
    say("  the two results are equal bit for bit: %s" % same)
    if not bar:
        say("  (no bar) composed %.3f ms against two-step %.3f ms" % (m1, m2))
        return same
    limit = m2 + s2_
    held = m1 <= limit
    say("  EXPECTATION %s: composed %.3f ms against the bar of %.3f ms (two-step mean %.3f ms + its spread %.3f ms)" % ("HELD" if held else "REFUTED", m1, limit, m2, s2_))
    mb, sb, _ = mean_spread(t["with_base"])
    mp, sp, _ = mean_spread(t["placed"])
    mw, sw_, _ = mean_spread(t["placed_whole"])
    cover_bytes = 3 * unowned * 2
    say("  cover kernel by difference: the composed call %.3f ms (spread %.3f); the same call with a whole-canvas base entry under each mosaic - no unowned pixel," % (m1, s1_))
    say("    no cover launch, but %d more entries of picture work over the same pixels - %.3f ms (spread %.3f): composed - based = %.3f ms%s" %
        (NC, mb, sb, m1 - mb, " - INSIDE the spread" if abs(m1 - mb) <= max(s1_, sb) else ""))
    if m1 - mb > max(s1_, sb):
        say("    the cover launch takes at least that: k_compose_cover writes its %d bytes at %.0f GB/s at the most" % (cover_bytes, cover_bytes / (m1 - mb) / 1e6))
    else:
        say("    no rate follows from it: the base entries' picture work takes as long as the cover launch over the same %d bytes, or longer" % cover_bytes)
    margin_bytes = 3 * NC * CANVAS * (CANVAS - rows) * 2
    say("  k_canvas_margin in the same run: a placed call of %d entries of %d x %d rows on the same canvases (%d margin bytes) %.3f ms (spread %.3f), with whole-canvas" %
        (NC, CANVAS, rows, margin_bytes, mp, sp))
    say("    rectangles (no margin launch) %.3f ms (spread %.3f): difference %.3f ms%s" % (mw, sw_, mp - mw, " - INSIDE the spread" if abs(mp - mw) <= max(sp, sw_) else ""))
    if mp - mw > max(sp, sw_):
        say("    (the whole-canvas call resizes %d more rows per entry) k_canvas_margin writes its bytes at %.0f GB/s at the most" % (CANVAS - rows, margin_bytes / (mp - mw) / 1e6))
    else:
        say("    no rate follows from it, as above")
    mc, sc_, _ = mean_spread(t["cover_only"])
    mm, sm, _ = mean_spread(t["margin_only"])
    say("  the direct pair, %d fill bytes each (the whole tensor but 16 x 16 pixels per canvas), the time of the whole call:" % tiny_bytes)
    say("    composed, four 8 x 8 entries per canvas: %.3f ms (spread %.3f) - k_compose_cover writes at %.0f GB/s at the least" % (mc, sc_, tiny_bytes / mc / 1e6))
    say("    placed, one 16 x 16 rectangle per canvas: %.3f ms (spread %.3f) - k_canvas_margin writes at %.0f GB/s at the least" % (mm, sm, tiny_bytes / mm / 1e6))
    say("    difference %.3f ms%s" % (mc - mm, " - INSIDE the spread" if abs(mc - mm) <= max(sc_, sm) else ""))
    try:
        import re
        sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
        from test_kernel_resources import _kernels
        step = lambda v: min(8, 512 // (8 * ((v + 7) // 8)))
        ks = _kernels()
        for dt, name in enumerate(("uint8", "float32", "float16", "bfloat16")):
            cv = [k for nm, k in ks.items() if re.search(r"\d+k_compose_coverILi%dEE" % dt, nm)][0]
            mg = [k for nm, k in ks.items() if re.search(r"\d+k_canvas_marginILi%dEE" % dt, nm)][0]
            say("  %-8s k_compose_cover %d VGPRs, %d waves / SIMD, LDS %d, scratch %d; k_canvas_margin %d VGPRs, %d waves / SIMD" %
                (name, cv["vgpr"], step(cv["vgpr"]), cv["lds"], cv["scratch"], mg["vgpr"], step(mg["vgpr"])))
    except BaseException as e:
        say("  kernel resources: not read (%s)" % (e,))
    return held and same

say("batch: %d generator stills (%d x %d, 8-bit 4:2:0), after run(); %d rounds, interleaved (the order alternates from round to round)" % (N, W, H, R))
say("expectation, written before the run: ONE composed call, BILINEAR, is not slower than the two-step way (to_tensor at %d x %d into scratch, one torch fill of" % (SW, SH))
say("the canvases, %d clipped slice copies) on the same build; the bar is the two-step way's mean plus its own max - min spread; bit-equal results are asserted" % n)
ok = shape("BILINEAR", decoder.SCALE_BILINEAR, True)
ok = shape("BOX", decoder.SCALE_BOX, False) and ok
ok = shape("BICUBIC", decoder.SCALE_BICUBIC, False) and ok
b.free()
say("")
say("done" if ok else "done: THE EXPECTATION WAS REFUTED, or two results differ (see above)")
