"""Packed tensor output against the way a host has without it, on one batch of 64 generator 4K stills (8-bit 4:2:0), all in one process on the same build,
interleaved rounds.  The workload is a native-resolution vision-language batch: 256 entries (four windows of different aspect ratio per still, orientation
codes 0 .. 7 in turn), each at its own aspect-preserving size of at most 1024 tokens of P = 14 with merge m = 2 (sides multiples of 28), float16, tokens in
Conv2d weight order, with BICUBIC and with BOX.  Two ways, both into torch tensors on one torch stream, timed by a pair of events on that stream around
everything a way enqueues; a few milliseconds of other work are put on the stream in front of the first event, so that a way's launches are queued before
the device reaches them and the time between the events is the device's:
 packed     ONE to_tensor_packed(patch=14, merge=2) call;
 today      one to_tensor(..., orientations=) per distinct size, torch reshape / permute of each result into tokens, one torch.cat.
The entries are ordered by size, so that the concatenation of the second way is the packed sequence of the first: the two results must be equal bit for bit.
Expectation to confirm or refute: the packed call is not slower at either filter (means over the rounds), and is faster by roughly the launch count.
Also measured: the packed call at P = 16 (4-pixel groups stay inside a patch: vector stores) against P = 14 (element stores), sizes by the same rule, and
the colour-stage device time of the packed calls (timing slot [5]).
A shape that misses the expectation is reported as such.  usage: python tools/measure_packed_output.py [report.txt] [--rehearse], from the repository root
after build(); --rehearse runs two small stills once through every call (no 4K streams needed, the numbers mean nothing)."""
import glob, math, os, sys
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
    say("not measured: torch sees no GPU (the way a host has today is made of torch calls)")
    sys.exit(1)

if REHEARSE:
    from oracle import pyoracle as orc
    W, H, N, TOKENS, R = 200, 136, 2, 16, 1
    streams = [orc.encode(orc.synth_image(W, H, 8, 1, seed=3 + i), bit_depth=8) for i in range(N)]
else:
    W, H, N, TOKENS, R = 3840, 2160, 64, 1024, 12
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
    """(device ms between two events on `side` around what `call` enqueues, slot-[5] us of the batch)"""
    with torch.cuda.stream(side):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(8):
            ballast.zero_()                                          # the device is busy while the host prepares and enqueues the calls
        e0.record(side); call(); e1.record(side)
    side.synchronize(); b.status()
    return e0.elapsed_time(e1), b.slot_kernel_timing_us(0)["colour"]

# four windows per still with aspect ratios spread between 1:2 and 2:1, odd offsets; codes 0 .. 7 in turn
rng = np.random.default_rng(11)
windows = []
for e in range(4 * N):
    r = float(np.exp(rng.uniform(np.log(0.5), np.log(2.0))))
    wh = int(min(H, W / r) * rng.uniform(0.6, 0.95))
    ww = min(W - 2, int(wh * r))
    windows.append((e % N, int(rng.integers(0, W - ww)) | 1, int(rng.integers(0, H - wh)) | 1, ww - 1, wh - 1, 0))
codes_all = [e % 8 for e in range(len(windows))]

def native_size(dw, dh, P, m):
    """the largest aspect-preserving size with sides multiples of P * m and at most TOKENS tokens (a plain rule for this tool: choosing sizes is the caller's)"""
    u = P * m
    s = math.sqrt(TOKENS * P * P / (dw * dh))
    return max(u, int(dw * s) // u * u), max(u, int(dh * s) // u * u)

def workload(P, m):
    sized = []
    for e, c in zip(windows, codes_all):
        dw, dh = (e[4], e[3]) if c & 1 else (e[3], e[4])
        sized.append((native_size(dw, dh, P, m), e, c))
    sized.sort(key=lambda t: t[0])                                    # by size: the concatenation of the per-size results is then the packed sequence
    return [t[0] for t in sized], [t[1] for t in sized], [t[2] for t in sized]

def tokens_of(t, P, m):
    """(k, 3, h, w) -> (k * tokens, 3 * P * P): the chain of the header for Conv2d weight order"""
    k, _, h, w = t.shape
    gh, gw = h // P, w // P
    return t.reshape(k, 3, gh // m, m, P, gw // m, m, P).permute(0, 2, 5, 3, 6, 1, 4, 7).reshape(k * gh * gw, 3 * P * P)

ok = True
def shape(fname, filt, P, m, against_today=True):
    global ok
    sizes, entries, codes = workload(P, m)
    n = len(entries)
    kw = dict(dtype="float16", layout="NCHW", mean=MEAN, std=STD, filter=filt)
    offsets, tokens, total = decoder.packed_layout(sizes, P, m)
    distinct = sorted(set(sizes))
    groups = [(s, [e for e in range(n) if sizes[e] == s]) for s in distinct]
    with torch.cuda.stream(side):
        packed = torch.empty((total,), dtype=torch.float16, device="cuda")
        scratch = [torch.empty((len(idx), 3, s[1], s[0]), dtype=torch.float16, device="cuda") for s, idx in groups]
    keep = {}
    def one_call():
        b.to_tensor_packed(sizes, entries, patch=P, merge=m, orientations=codes, offsets=offsets, out=packed, **kw)
    def today():
        parts = []
        for (s, idx), t in zip(groups, scratch):
            b.to_tensor(s, [entries[e] for e in idx], out=t, orientations=[codes[e] for e in idx], **kw)
            parts.append(tokens_of(t, P, m))
        keep["seq"] = torch.cat(parts)
    ways = (one_call, today) if against_today else (one_call,)
    for c in ways:
        for _ in range(1 if REHEARSE else 2):
            timed(c)
    t1, t2, s5 = [], [], []
    for r in range(R):
        for c in (ways if r % 2 == 0 else ways[::-1]):
            ms, us = timed(c)
            if c is one_call:
                t1.append(ms); s5.append(us)
            else:
                t2.append(ms)
    t1, s5 = np.array(t1), np.array(s5)
    say("")
    say("%s, P = %d, m = %d: %d entries, %d distinct sizes, %d tokens x %d float16 = %.1f MB" % (fname, P, m, n, len(distinct), sum(tokens), 3 * P * P, total * 2 / 1e6))
    say("  packed, one call                            events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f   slot [5] mean %8.1f us  min %8.1f  max %8.1f" %
        (t1.mean(), np.median(t1), t1.min(), t1.max(), s5.mean(), s5.min(), s5.max()))
    if not against_today:
        return t1
    t2 = np.array(t2)
    same = bool(torch.equal(keep["seq"].reshape(-1), packed))
    say("  today: %3d x to_tensor + %3d x reshape / permute + cat  events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f" % (len(distinct), len(distinct), t2.mean(), np.median(t2), t2.min(), t2.max()))
    good = t1.mean() <= t2.mean()
    say("  packed against today: %.3f ms against %.3f ms (%.1f x): %s" % (t1.mean(), t2.mean(), t2.mean() / t1.mean(), "not slower" if good else "SLOWER"))
    say("  the two results are equal bit for bit: %s" % same)
    ok = ok and good and same
    return t1

say("batch: %d generator stills (%d x %d, 8-bit 4:2:0), after run(); %d entries, at most %d tokens each; %d rounds, interleaved (the order alternates from round to round)" %
    (N, W, H, len(windows), TOKENS, R))
P14 = {}
for fname, filt in (("BICUBIC", decoder.SCALE_BICUBIC), ("BOX", decoder.SCALE_BOX)):
    P14[fname] = shape(fname, filt, 14, 2)
say("")
say("vector-store path (P = 16) against the element path (P = 14), the packed call alone:")
for fname, filt in (("BICUBIC", decoder.SCALE_BICUBIC), ("BOX", decoder.SCALE_BOX)):
    t16 = shape(fname, filt, 16, 2, against_today=False)
    say("  %s: P = 16 %.3f ms against P = 14 %.3f ms (means)" % (fname, t16.mean(), P14[fname].mean()))
b.free()
say("done" if ok else "done: AN EXPECTATION WAS MISSED (see above)")
