"""Placed tensor output against the two-step way a host has without it, on one batch of 64 generator 4K stills (8-bit 4:2:0), all in one process on the same
build, interleaved rounds.  Two shapes:
 letterbox  64 stills -> 640 x 640 float16 NCHW, the picture as 640 x 360 in the middle, fill 114 (component domain), with BOX and BILINEAR;
 padded     256 windows (four per still: 1:1, 4:3, 3:4 and 16:9) -> 224 x 224 float16 NCHW, each letterboxed by its own aspect, fill 114, BOX.
Two ways, both into torch tensors on one torch stream, timed by a pair of events on that stream around everything a way enqueues.  A few milliseconds of
other work are put on the stream in front of the first event, so that a way's launches are queued before the device reaches them: the time between the events
is the device's, not the host's preparation of the calls:
 placed     ONE to_tensor(places=, fill=) call: the picture launch and the margin launch;
 two-step   to_tensor per distinct rectangle size into a scratch tensor, one fill pass over the canvas (torch.full's cost; a broadcast copy, as the three
            fill elements differ), one slice copy per size.
Expectation to confirm or refute: the placed call is not slower than the two-step way at either shape (means over the rounds).
Also reported: the placed call's colour-stage device time (timing slot [5]: the picture launch and the margin launch), the same slot summed over the
existing oriented call (code 0: the same picture kernel) per rectangle size into dense scratch tensors, and the margin kernel's written bytes over the
difference of the two.
A shape that misses the expectation is reported as such.  usage: python tools/measure_placed_output.py [report.txt] [--rehearse], from the repository root
after build(); --rehearse runs two small stills once through every call (no 4K streams needed, the numbers mean nothing)."""
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
    W, H, N, LB, TS, R = 200, 136, 2, 64, 24, 1
    streams = [orc.encode(orc.synth_image(W, H, 8, 1, seed=3 + i), bit_depth=8) for i in range(N)]
else:
    W, H, N, LB, TS, R = 3840, 2160, 64, 640, 224, 12
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
SC, BI = decoder.tensor_scale_bias(MEAN, STD)
FILL = 114
fill_elems = (np.float32(FILL) * SC + BI).astype(np.float16)           # the component domain's definition, restated
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

def shape(title, canvas, entries, places, filt, fname):
    """one shape: the placed call against the two-step way, R interleaved rounds"""
    global ok
    n = len(entries)
    cw, ch = canvas
    kw = dict(dtype="float16", layout="NCHW", mean=MEAN, std=STD, filter=filt)
    sizes = sorted(set(p[2:] for p in places))
    groups = [(s, [e for e in range(n) if places[e][2:] == s]) for s in sizes]
    for s, idx in groups:                                            # a slice copy per size needs the entries of a size side by side, at one offset
        assert idx == list(range(idx[0], idx[0] + len(idx))) and len(set(places[e][:2] for e in idx)) == 1
    with torch.cuda.stream(side):
        placed = torch.empty((n, 3, ch, cw), dtype=torch.float16, device="cuda")
        scratch = [torch.empty((len(idx), 3, s[1], s[0]), dtype=torch.float16, device="cuda") for s, idx in groups]
        fill_t = torch.from_numpy(fill_elems).cuda().view(1, 3, 1, 1)
    keep = {}
    def one_call():
        b.to_tensor(canvas, entries, places=places, fill=FILL, out=placed, **kw)
    def two_step():
        for (s, idx), t in zip(groups, scratch):
            b.to_tensor(s, [entries[e] for e in idx], out=t, **kw)
        c = torch.empty((n, 3, ch, cw), dtype=torch.float16, device="cuda")
        c[:] = fill_t                                                # (torch.full's one pass over the canvas; a broadcast copy, since the three fill elements differ)
        for (s, idx), t in zip(groups, scratch):
            x, y = places[idx[0]][:2]
            c[idx[0]:idx[0] + len(idx), :, y:y + s[1], x:x + s[0]] = t
        keep["c"] = c
    def dense_oriented_us():
        us = 0.0
        for (s, idx), t in zip(groups, scratch):
            b.to_tensor(s, [entries[e] for e in idx], out=t, orientations=[0] * len(idx), **kw)
            side.synchronize(); b.status()
            us += b.slot_kernel_timing_us(0)["colour"]
        return us
    with torch.cuda.stream(side):
        dense_oriented_us()
    for c in (one_call, two_step):
        for _ in range(1 if REHEARSE else 2):
            timed(c)
    t1, t2, s5, tm = [], [], [], []
    for r in range(R):
        for c, ev, slot in ((one_call, t1, s5), (two_step, t2, None)) if r % 2 == 0 else ((two_step, t2, None), (one_call, t1, s5)):
            ms, us = timed(c)
            ev.append(ms)
            if slot is not None:
                slot.append(us)
    same = bool(torch.equal(keep["c"], placed))
    with torch.cuda.stream(side):
        for r in range(R):
            tm.append(dense_oriented_us())
    t1, t2, s5, tm = np.array(t1), np.array(t2), np.array(s5), np.array(tm)
    margin_bytes = sum(3 * (cw * ch - p[2] * p[3]) * 2 for p in places)
    all_bytes = n * 3 * cw * ch * 2
    say("")
    say("%s, %s: %d entries -> %d x %d float16 NCHW, %d distinct rectangle size(s); canvas %.1f MB, of it margin %.1f MB" % (title, fname, n, cw, ch, len(sizes), all_bytes / 1e6, margin_bytes / 1e6))
    say("  placed, one call                                   events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f   slot [5] mean %8.1f us  min %8.1f  max %8.1f" %
        (t1.mean(), np.median(t1), t1.min(), t1.max(), s5.mean(), s5.min(), s5.max()))
    say("  two-step: %d x to_tensor + canvas fill + %d slice copies  events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f" % (len(sizes), len(sizes), t2.mean(), np.median(t2), t2.min(), t2.max()))
    good = t1.mean() <= t2.mean()
    say("  placed against two-step: %.3f ms against %.3f ms: %s" % (t1.mean(), t2.mean(), "not slower" if good else "SLOWER"))
    say("  the two results are equal bit for bit: %s" % same)
    diff = s5.mean() - tm.mean()
    say("  the picture kernel alone (oriented call, code 0, dense, per size): slot [5] sum mean %8.1f us  min %8.1f  max %8.1f" % (tm.mean(), tm.min(), tm.max()))
    say("  margin launch, by difference: %.1f us for %.1f MB of margin -> %s" % (diff, margin_bytes / 1e6, "%.3f TB/s" % (margin_bytes / diff / 1e6) if diff > 0 else "inside the spread"))
    ok = ok and good and same

ok = True
say("batch: %d generator stills (%d x %d, 8-bit 4:2:0), after run(); %d rounds, interleaved (the order alternates from round to round)" % (N, W, H, R))
whole = [(i, 0, 0, 0, 0, 0) for i in range(N)]
lb = decoder.letterbox_places([(W, H)] * N, (LB, LB))
for fname, filt in (("BOX", decoder.SCALE_BOX), ("BILINEAR", decoder.SCALE_BILINEAR)):
    shape("letterbox", (LB, LB), whole, lb, filt, fname)
# four windows per still, grouped by aspect so that the two-step way has one slice copy per size
wins = []
for aw, ah in ((1, 1), (4, 3), (3, 4), (16, 9)):
    u = min(W // aw, H // ah) * 3 // 4
    ww, wh = u * aw, u * ah
    wins += [(i, (W - ww) // 2 | 1, (H - wh) // 2 | 1, ww, wh, 0) for i in range(N)]
shape("padded", (TS, TS), wins, decoder.letterbox_places([(e[3], e[4]) for e in wins], (TS, TS)), decoder.SCALE_BOX, "BOX")
say("")
say("context, not a bar: the album paste kernel writes at 5.3 TB/s (profiles/album.txt)")
b.free()
say("done" if ok else "done: AN EXPECTATION WAS MISSED (see above)")
