"""Framed tensor output against the two-step way a host has without it, on one batch of 64 generator 4K stills (8-bit 4:2:0), all in one process on the same
build, interleaved rounds: torchvision's evaluation pipeline Resize(256) -> CenterCrop(224) as a float16 NCHW batch of 256 entries (every still four times,
two of them flipped), with BICUBIC - the bar - and, beside it without a bar, BILINEAR and BOX.
Two ways, both into torch tensors on one torch stream, timed by a pair of events on that stream around everything a way enqueues.  A few milliseconds of
other work are put on the stream in front of the first event, so that a way's launches are queued before the device reaches them: the time between the events
is the device's, not the host's preparation of the calls:
 framed     ONE to_tensor(frames=resize_crop_places(...)) call: the k_frame_* launch (no margin: the resized sample covers the canvas);
 two-step   to_tensor at the resized size (455 x 256) into a scratch tensor, then x[..., y:y + 224, x:x + 224].contiguous() with the SAME offsets
            (hipdec_resize_crop_place's: round half to even, as torchvision's CenterCrop), so that the results can be compared bit for bit.
Expectation, written into the report BEFORE the run: one framed call is not slower than the two-step way.  The bar is the two-step way's mean plus its own
max - min spread over the rounds (differences below a call's spread are indications only); HELD or REFUTED is reported with both figures.
Also reported: the share of the pieces of work skipped (hipdec_framed_stats), the framed call's colour-stage device time (timing slot [5]) and the same slot
of the two-step way's to_tensor - the kernel alone, so that a refuted bar names the kernel that carries the difference (the rest is the slice copy).
usage: python tools/measure_framed_output.py [report.txt] [--rehearse], from the repository root after build(); --rehearse runs two small stills once through
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
    W, H, N, PER, RESIZE, CROP, R = 200, 136, 2, 2, 32, 28, 1
    streams = [orc.encode(orc.synth_image(W, H, 8, 1, seed=3 + i), bit_depth=8) for i in range(N)]
else:
    W, H, N, PER, RESIZE, CROP, R = 3840, 2160, 64, 4, 256, 224, 12
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
    """(device ms between two events on `side` around what `call` enqueues, slot-[5] us of the batch's last colour-stage call)"""
    with torch.cuda.stream(side):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(8):
            ballast.zero_()                                          # the device is busy while the host prepares and enqueues the calls
        e0.record(side); call(); e1.record(side)
    side.synchronize(); b.status()
    return e0.elapsed_time(e1), b.slot_kernel_timing_us(0)["colour"]

n = N * PER
entries = [(i % N, 0, 0, 0, 0, (i // N) & 1) for i in range(n)]
frame = decoder.resize_crop_place((W, H), RESIZE, (CROP, CROP))
fx, fy, rw, rh = frame
assert fx <= 0 and fy <= 0 and fx + rw >= CROP and fy + rh >= CROP, frame    # the resized sample covers the canvas: no margin launch
frames = [frame] * n

def shape(fname, filt, bar):
    kw = dict(dtype="float16", layout="NCHW", mean=MEAN, std=STD, filter=filt)
    with torch.cuda.stream(side):
        framed = torch.empty((n, 3, CROP, CROP), dtype=torch.float16, device="cuda")
        scratch = torch.empty((n, 3, rh, rw), dtype=torch.float16, device="cuda")
    keep = {}
    def one_call():
        b.to_tensor((CROP, CROP), entries, frames=frames, out=framed, **kw)
    def two_step():
        b.to_tensor((rw, rh), entries, out=scratch, **kw)
        keep["c"] = scratch[..., -fy:-fy + CROP, -fx:-fx + CROP].contiguous()
    s0 = decoder.framed_stats()
    for c in (one_call, two_step):
        for _ in range(1 if REHEARSE else 2):
            timed(c)
    s1 = decoder.framed_stats()
    calls, tiles, skipped = s1[0] - s0[0], s1[2] - s0[2], s1[3] - s0[3]
    t1, t2, k1, k2 = [], [], [], []
    for r in range(R):
        for c, ev, slot in ((one_call, t1, k1), (two_step, t2, k2)) if r % 2 == 0 else ((two_step, t2, k2), (one_call, t1, k1)):
            ms, us = timed(c)
            ev.append(ms); slot.append(us)
    same = bool(torch.equal(keep["c"], framed))
    t1, t2, k1, k2 = np.array(t1), np.array(t2), np.array(k1), np.array(k2)
    say("")
    say("%s: %d entries, Resize(%d) -> %d x %d, CenterCrop(%d) at (%d, %d), float16 NCHW; computed and written by the two-step way %d x %d pixels per entry, kept %d x %d (%.0f %%)" %
        (fname, n, RESIZE, rw, rh, CROP, -fx, -fy, rw, rh, CROP, CROP, 100.0 * CROP * CROP / (rw * rh)))
    say("  framed, one call                      events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f   slot [5] mean %8.1f us  min %8.1f  max %8.1f" %
        (t1.mean(), np.median(t1), t1.min(), t1.max(), k1.mean(), k1.min(), k1.max()))
    say("  two-step: to_tensor + slice copy      events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f   slot [5] mean %8.1f us  min %8.1f  max %8.1f (the to_tensor alone)" %
        (t2.mean(), np.median(t2), t2.min(), t2.max(), k2.mean(), k2.min(), k2.max()))
    say("  pieces of work per framed call: %d with a visible pixel, %d skipped (%.0f %% skipped)" % (tiles // max(calls, 1), skipped // max(calls, 1), 100.0 * skipped / max(tiles + skipped, 1)))
    say("  the two results are equal bit for bit: %s" % same)
    limit = t2.mean() + (t2.max() - t2.min())
    if bar:
        held = t1.mean() <= limit
        say("  EXPECTATION %s: framed %.3f ms against the bar of %.3f ms (two-step mean %.3f ms + its spread %.3f ms)" % ("HELD" if held else "REFUTED", t1.mean(), limit, t2.mean(), t2.max() - t2.min()))
        if not held:
            say("  the difference by kernel: k_frame_resample %.1f us against k_resample at the full rectangle %.1f us; the slice copy, by difference, %.1f us" %
                (k1.mean(), k2.mean(), t2.mean() * 1e3 - k2.mean()))
        return held and same
    say("  (no bar) framed %.3f ms against two-step %.3f ms" % (t1.mean(), t2.mean()))
    return same

say("batch: %d generator stills (%d x %d, 8-bit 4:2:0), after run(); %d rounds, interleaved (the order alternates from round to round)" % (N, W, H, R))
say("expectation, written before the run: ONE framed call, BICUBIC, is not slower than the two-step way (to_tensor at the resized size into scratch, then a slice")
say("copy) on the same build; the bar is the two-step way's mean plus its own max - min spread; bit-equal results are asserted")
ok = shape("BICUBIC", decoder.SCALE_BICUBIC, True)
ok = shape("BILINEAR", decoder.SCALE_BILINEAR, False) and ok
ok = shape("BOX", decoder.SCALE_BOX, False) and ok
b.free()
say("")
say("done" if ok else "done: THE EXPECTATION WAS REFUTED, or two results differ (see above)")
