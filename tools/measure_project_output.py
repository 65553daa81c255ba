"""Projective tensor output (hipdec_batch_to_tensor_projected, k_project_*) on the warp section's workload (tools/measure_warp_output.py): one batch of 64
generator 4K stills (8-bit 4:2:0), 256 random-resized-crop windows (four per still) resized with BILINEAR to 224 x 224, float16 NCHW with the ImageNet mean
/ std, fill 0.  All in one process on one build, 12 interleaved rounds, for the filters NEAREST, BILINEAR and BICUBIC.  Two sets of maps:
  affine       the warp section's rotations (+-30 degrees about the centre) as PERSPECTIVE maps with a6 = a7 = 0, beside the warped call with the same
               rotations: the two calls differ in the coordinate function alone (two fp64 divisions per pixel, by 1.0) and - NEAREST - in Pillow's path;
  perspective  RandomPerspective-style maps: torchvision's get_params with distortion_scale 0.5 drawn with a fixed seed from NumPy, through
               decoder.perspective_map.

Expectations, stated before the run:
 (a) device time, between two events on one torch stream around what a way enqueues (a few milliseconds of other work are queued in front of the first
     event, so that the launches wait in the queue and the time is the device's).  The cost of the projective launch is taken by difference against the
     unwarped to_tensor call for the same entries and resize filter, and put beside the warped call's cost taken the same way.  NO BAR: nobody has measured
     what two fp64 divisions per pixel cost on this chip, so nothing is promised; reported are the two costs, their difference and ratio, and whether the
     difference exceeds the spread (max - min) of the calls it is taken from.  The BILINEAR / BICUBIC results of the affine maps and of the warped call are
     equal bit for bit (asserted).
 (b) wall clock around a synchronise, perspective maps: the projected call is far below the host way - to_tensor "uint8" NHWC, tensor_to_host,
     PIL.Image.transform(PERSPECTIVE) per sample, upload of the 8-bit result (the host way is not even normalised) - "far" being at least 10 x for BILINEAR
     and BICUBIC, the warp section's own bar; NEAREST is reported without a bar (the warp section's NEAREST reached 8.5 x and was refuted).  The two 8-bit
     results are equal bit for bit (asserted, all three filters).
BILINEAR and BICUBIC report HELD or REFUTED for (b) with the numbers.
usage: python tools/measure_project_output.py [report.txt] [--rehearse], from the repository root after build(); --rehearse runs two small stills once
through every call (no 4K streams needed, the numbers mean nothing)."""
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
rotations = [decoder.rotate_matrix(float(a), (TS, TS)) for a in angles]
affine = [tuple(m) + (0.0, 0.0) for m in rotations]

def random_perspective(rng, w, h, distortion=0.5):
    """torchvision.transforms.RandomPerspective.get_params: (startpoints, endpoints)"""
    hw, hh = int(distortion * (w // 2)), int(distortion * (h // 2))
    tl = (int(rng.integers(0, hw + 1)), int(rng.integers(0, hh + 1)))
    tr = (int(rng.integers(w - hw - 1, w)), int(rng.integers(0, hh + 1)))
    br = (int(rng.integers(w - hw - 1, w)), int(rng.integers(h - hh - 1, h)))
    bl = (int(rng.integers(0, hw + 1)), int(rng.integers(h - hh - 1, h)))
    return [(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)], [tl, tr, br, bl]

prng = np.random.default_rng(50)
perspective = [tuple(decoder.perspective_map(*random_perspective(prng, TS, TS)).a) for _ in range(n)]
RESIZE = decoder.SCALE_BILINEAR
kw = dict(dtype="float16", layout="NCHW", mean=MEAN, std=STD, filter=RESIZE)
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    ballast = torch.empty(64 << 20 if REHEARSE else 512 << 20, dtype=torch.uint8, device="cuda")
    plain = torch.empty((n, 3, TS, TS), dtype=torch.float16, device="cuda")
    warped = torch.empty((n, 3, TS, TS), dtype=torch.float16, device="cuda")
    proj_a = torch.empty((n, 3, TS, TS), dtype=torch.float16, device="cuda")
    proj_p = torch.empty((n, 3, TS, TS), dtype=torch.float16, device="cuda")
    proj8 = torch.empty((n, TS, TS, 3), dtype=torch.uint8, device="cuda")
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

say("expectation (a): none promised - the cost of the projective launch, by difference against the unwarped to_tensor call, beside the warped call's cost for the "
    "same rotations (a6 = a7 = 0); reported: both costs, difference, ratio, and whether the difference exceeds the spread of the calls it is taken from; the BILINEAR / "
    "BICUBIC results of the two calls are equal bit for bit")
say("expectation (b): one to_tensor_projected call (RandomPerspective maps), wall clock around a synchronise, is at least 10 x below the host way (to_tensor uint8, "
    "tensor_to_host, PIL.Image.transform(PERSPECTIVE) per sample, upload) for BILINEAR and BICUBIC; NEAREST without a bar; the 8-bit results are equal bit for bit")
try:                                                                 # the compiled resources of the kernels measured, from the code objects of the library loaded
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    from test_project_kernel_resources import _project_kernels
    ks = _project_kernels()
    say("compiled (gfx950), VGPRs for U8 / F32 / F16 / BF16, scratch and LDS bytes over all: " + "; ".join(
        "k_project_%s %s, %d, %d" % (f, " / ".join(str(ks[(f, d)]["vgpr"]) for d in range(4)), max(ks[(f, d)]["scratch"] for d in range(4)),
                                     max(ks[(f, d)]["lds"] for d in range(4))) for f in ("nearest", "bilinear", "bicubic")))
except Exception as e:
    say("compiled resources: not read (%s)" % e)
say("")
say("batch: %d generator stills (%d x %d, 8-bit 4:2:0), after run(); %d random-resized-crop windows -> %d x %d float16 NCHW, resize BILINEAR; affine maps: rotations "
    "from +-30 degrees with a6 = a7 = 0; perspective maps: RandomPerspective's, distortion 0.5, seed 50; %d rounds, interleaved (the order rotates from round to round)"
    % (N, W, H, n, TS, TS, R))
ok = True
for fname, wf, pil in (("NEAREST", decoder.SCALE_NEAREST, "NEAREST"), ("BILINEAR", decoder.SCALE_BILINEAR, "BILINEAR"), ("BICUBIC", decoder.SCALE_BICUBIC, "BICUBIC")):
    def unwarped():
        b.to_tensor((TS, TS), entries, out=plain, **kw)
    def warp_call():
        b.to_tensor_warped((TS, TS), rotations, entries, warp_filter=wf, fill=0, out=warped, **kw)
    def project_affine():
        b.to_tensor_projected((TS, TS), affine, entries, warp_filter=wf, fill=0, out=proj_a, **kw)
    def project_perspective():
        b.to_tensor_projected((TS, TS), perspective, entries, warp_filter=wf, fill=0, out=proj_p, **kw)
    def project8():
        b.to_tensor_projected((TS, TS), perspective, entries, warp_filter=wf, fill=0, out=proj8, dtype="uint8", layout="NHWC", filter=RESIZE)
        return proj8
    def host_way():
        b.to_tensor((TS, TS), entries, out=mid8, dtype="uint8", layout="NHWC", filter=RESIZE)
        host = b.tensor_to_host()
        res = np.stack([np.asarray(Image.fromarray(host[e]).transform((TS, TS), Image.Transform.PERSPECTIVE, data=perspective[e], resample=getattr(Image, pil),
                                                                      fillcolor=(0, 0, 0))) for e in range(n)])
        return torch.from_numpy(res).to("cuda", non_blocking=False)
    ways = [unwarped, warp_call, project_affine, project_perspective]
    for c in ways:
        for _ in range(1 if REHEARSE else 2):
            timed(c)
    t = [[] for _ in ways]
    for r in range(R):
        for k in range(len(ways)):
            i = (k + r) % len(ways)
            t[i].append(timed(ways[i]))
    t = [np.array(v) for v in t]
    say("")
    say("filter %s" % fname)
    for name, v in zip(("to_tensor (unwarped)", "to_tensor_warped, rotations", "to_tensor_projected, affine", "to_tensor_projected, perspective"), t):
        say("  %-34s events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f" % (name, v.mean(), np.median(v), v.min(), v.max()))
    cw, ca, cp = t[1].mean() - t[0].mean(), t[2].mean() - t[0].mean(), t[3].mean() - t[0].mean()
    spread = max(v.max() - v.min() for v in t[:3])
    say("  (a) by difference against the unwarped call: warp stage %.3f ms, projective stage %.3f ms with the same maps (difference %+.3f ms, ratio %.2f), %.3f ms "
        "with the perspective maps" % (cw, ca, ca - cw, ca / cw if cw > 0 else float("nan"), cp))
    say("      the largest spread (max - min) of the calls the difference is taken from is %.3f ms: the difference %s it" %
        (spread, "exceeds" if abs(ca - cw) > spread else "does not exceed"))
    if wf != decoder.SCALE_NEAREST:
        side.synchronize()
        same = bool(torch.equal(warped.view(torch.int16), proj_a.view(torch.int16)))
        assert same, "the projected call with a6 = a7 = 0 and the warped call differ (%s)" % fname
        say("      the results of the affine maps and of the warped call are equal bit for bit: %s" % same)
    w1 = np.array([wall(project_perspective)[0] for _ in range(R)])
    say("  to_tensor_projected, perspective, wall clock around a synchronise: mean %8.3f ms  min %8.3f  max %8.3f" % (w1.mean(), w1.min(), w1.max()))
    if Image is None:
        say("  (b) not measured: Pillow is not installed")
        ok = False
        continue
    hw = []
    for _ in range(1 if REHEARSE else 3):
        ms, res = wall(host_way)
        hw.append(ms)
    hw = np.array(hw)
    _, got8 = wall(project8)
    same = bool(torch.equal(res, got8))
    assert same, "the projected call and PIL.Image.transform differ (%s)" % fname
    say("  host way (to_tensor uint8, tensor_to_host, PIL transform per sample, upload), wall clock: mean %8.3f ms  min %8.3f  max %8.3f" % (hw.mean(), hw.min(), hw.max()))
    if wf == decoder.SCALE_NEAREST:
        say("  (b) projected %.3f ms against the host way %.3f ms (%.1f x): no bar for NEAREST; the two 8-bit results are equal bit for bit: %s" %
            (w1.mean(), hw.mean(), hw.mean() / w1.mean(), same))
        continue
    far = w1.mean() * 10 <= hw.mean()
    say("  (b) projected %.3f ms against the host way %.3f ms (%.1f x): %s; the two 8-bit results are equal bit for bit: %s" %
        (w1.mean(), hw.mean(), hw.mean() / w1.mean(), "HELD" if far else "REFUTED (less than 10 x)", same))
    ok = ok and far
b.free()
say("")
say("done" if ok else "done: AN EXPECTATION WAS MISSED (see above)")
