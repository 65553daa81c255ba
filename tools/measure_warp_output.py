"""Warped tensor output (hipdec_batch_to_tensor_warped, k_warp_*) on one batch of 64 generator 4K stills (8-bit 4:2:0): 256 random-resized-crop windows
(four per still) resized with BILINEAR to 224 x 224 and rotated about the centre by an angle drawn uniformly from +-30 degrees, float16 NCHW with the
ImageNet mean / std, fill 0.  All in one process on one build, 12 interleaved rounds, for the warp filters NEAREST, BILINEAR and BICUBIC.

Expectations, stated before the run:
 (a) device time, between two events on one torch stream around what a way enqueues (a few milliseconds of other work are queued in front of the first
     event, so that the launches wait in the queue and the time is the device's): the warped call is within the unwarped to_tensor call's time for the same
     entries and resize filter PLUS the time of one dense pass over the intermediate (256 x 224 x 224 x 3 bytes) and the output (256 x 3 x 224 x 224 x 2
     bytes) at the 0.9 TB/s at which k_canvas_margin writes its margins (profiles/placed_output.txt);
 (b) wall clock around a synchronise: the warped call is far below the host way - to_tensor "uint8" NHWC, tensor_to_host, PIL.Image.transform per sample,
     upload of the 8-bit result (the host way is not even normalised) - "far" being at least 10 x - and the two 8-bit results are equal bit for bit
     (asserted).
Each filter reports HELD or REFUTED with the numbers.
usage: python tools/measure_warp_output.py [report.txt] [--rehearse], from the repository root after build(); --rehearse runs two small stills once through
every call (no 4K streams needed, the numbers mean nothing)."""
import glob, os, sys, time
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
    say("not measured: torch sees no GPU (the events and the output tensors are torch's)")
    sys.exit(1)
try:
    from PIL import Image
except Exception:
    Image = None

if REHEARSE:
    from oracle import pyoracle as orc
    W, H, N, PER, TS, R = 200, 136, 2, 2, 24, 1
    streams = [orc.encode(orc.synth_image(W, H, 8, 1, seed=3 + i), bit_depth=8) for i in range(N)]
else:
    W, H, N, PER, TS, R = 3840, 2160, 64, 4, 224, 12
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
rng = np.random.default_rng(2026)
entries = decoder.random_resized_crop_entries(rng, [(W, H)] * (N * PER), items=[i % N for i in range(N * PER)])
n = len(entries)
angles = rng.uniform(-30.0, 30.0, n)
maps = [decoder.rotate_matrix(float(a), (TS, TS)) for a in angles]
RESIZE = decoder.SCALE_BILINEAR
kw = dict(dtype="float16", layout="NCHW", mean=MEAN, std=STD, filter=RESIZE)
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    ballast = torch.empty(64 << 20 if REHEARSE else 512 << 20, dtype=torch.uint8, device="cuda")
    plain = torch.empty((n, 3, TS, TS), dtype=torch.float16, device="cuda")
    warped = torch.empty((n, 3, TS, TS), dtype=torch.float16, device="cuda")
    warped8 = torch.empty((n, TS, TS, 3), dtype=torch.uint8, device="cuda")
    mid8 = torch.empty((n, TS, TS, 3), dtype=torch.uint8, device="cuda")

def timed(call):
    """device ms between two events on `side` around what `call` enqueues"""
    with torch.cuda.stream(side):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(8):
            ballast.zero_()                                          # the device is busy while the host prepares and enqueues the calls
        e0.record(side); call(); e1.record(side)
    side.synchronize(); b.status()
    return e0.elapsed_time(e1)

def wall(call):
    """wall-clock ms of `call` and a synchronise behind it, from an idle device"""
    side.synchronize(); b.status()
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        r = call()
    side.synchronize()
    return (time.perf_counter() - t0) * 1e3, r

PASS_BYTES = n * TS * TS * 3 + n * 3 * TS * TS * 2
PASS_MS = PASS_BYTES / 0.9e12 * 1e3
say("batch: %d generator stills (%d x %d, 8-bit 4:2:0), after run(); %d random-resized-crop windows -> %d x %d float16 NCHW, resize BILINEAR, rotations from +-30 degrees; "
    "%d rounds, interleaved (the order alternates from round to round)" % (N, W, H, n, TS, TS, R))
say("one dense pass over the intermediate and the output: %.1f MB, %.3f ms at 0.9 TB/s (k_canvas_margin's rate, profiles/placed_output.txt)" % (PASS_BYTES / 1e6, PASS_MS))
ok = True
for fname, wf, pil in (("NEAREST", decoder.SCALE_NEAREST, "NEAREST"), ("BILINEAR", decoder.SCALE_BILINEAR, "BILINEAR"), ("BICUBIC", decoder.SCALE_BICUBIC, "BICUBIC")):
    def unwarped():
        b.to_tensor((TS, TS), entries, out=plain, **kw)
    def one_call():
        b.to_tensor_warped((TS, TS), maps, entries, warp_filter=wf, fill=0, out=warped, **kw)
    def one_call8():
        b.to_tensor_warped((TS, TS), maps, entries, warp_filter=wf, fill=0, out=warped8, dtype="uint8", layout="NHWC", filter=RESIZE)
        return warped8
    def host_way():
        b.to_tensor((TS, TS), entries, out=mid8, dtype="uint8", layout="NHWC", filter=RESIZE)
        host = b.tensor_to_host()
        res = np.stack([np.asarray(Image.fromarray(host[e]).transform((TS, TS), Image.AFFINE, data=maps[e], resample=getattr(Image, pil), fillcolor=(0, 0, 0)))
                        for e in range(n)])
        return torch.from_numpy(res).to("cuda", non_blocking=False)
    for c in (unwarped, one_call):
        for _ in range(1 if REHEARSE else 2):
            timed(c)
    t0, t1 = [], []
    for r in range(R):
        for c, ev in ((unwarped, t0), (one_call, t1)) if r % 2 == 0 else ((one_call, t1), (unwarped, t0)):
            ev.append(timed(c))
    t0, t1 = np.array(t0), np.array(t1)
    say("")
    say("warp filter %s" % fname)
    say("  to_tensor (unwarped)        events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f" % (t0.mean(), np.median(t0), t0.min(), t0.max()))
    say("  to_tensor_warped, one call  events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f" % (t1.mean(), np.median(t1), t1.min(), t1.max()))
    held = t1.mean() <= t0.mean() + PASS_MS
    say("  (a) warped %.3f ms against unwarped %.3f ms + one pass %.3f ms = %.3f ms: %s (the warp stage costs %.3f ms, %.2f passes)" %
        (t1.mean(), t0.mean(), PASS_MS, t0.mean() + PASS_MS, "HELD" if held else "REFUTED", t1.mean() - t0.mean(), (t1.mean() - t0.mean()) / PASS_MS))
    ok = ok and held
    w1 = np.array([wall(one_call)[0] for _ in range(R)])
    say("  to_tensor_warped, wall clock around a synchronise: mean %8.3f ms  min %8.3f  max %8.3f" % (w1.mean(), w1.min(), w1.max()))
    if Image is None:
        say("  (b) not measured: Pillow is not installed")
        ok = False
        continue
    hw = []
    for _ in range(1 if REHEARSE else 3):
        ms, res = wall(host_way)
        hw.append(ms)
    hw = np.array(hw)
    _, got8 = wall(one_call8)
    same = bool(torch.equal(res, got8))
    assert same, "the warped call and PIL.Image.transform differ (%s)" % fname
    far = w1.mean() * 10 <= hw.mean()
    say("  host way (to_tensor uint8, tensor_to_host, PIL transform per sample, upload), wall clock: mean %8.3f ms  min %8.3f  max %8.3f" % (hw.mean(), hw.min(), hw.max()))
    say("  (b) warped %.3f ms against the host way %.3f ms (%.0f x): %s; the two 8-bit results are equal bit for bit: %s" %
        (w1.mean(), hw.mean(), hw.mean() / w1.mean(), "HELD" if far else "REFUTED (less than 10 x)", same))
    ok = ok and far
b.free()
say("")
say("done" if ok else "done: AN EXPECTATION WAS MISSED (see above)")
