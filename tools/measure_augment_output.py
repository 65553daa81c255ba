"""Augmented tensor output (hipdec_batch_to_tensor_augmented, k_augment_hue / k_augment_blur beside the photo kernels) on one batch of 64 generator 4K
stills (8-bit 4:2:0): 256 random-resized-crop windows (four per still) resized with BILINEAR to 224 x 224, float16 NCHW with the ImageNet mean / std.
All in one process on one build, 12 interleaved rounds.

Expectations, written into the report before anything is measured:
 (a) device time, between two events on one torch stream around what a way enqueues (a few milliseconds of other work are queued in front of the first
     event, so that the launches wait in the queue and the time is the device's): the augmented call with a one-step GAUSSIAN_BLUR chain of radius 2
     costs no more than the existing to_tensor call for the same entries PLUS SIX dense passes over the intermediate, each reading and writing
     256 x 224 x 224 x 3 bytes - the floor of doing the six box passes as separate launches through memory -, priced at the rate k_canvas_margin
     reaches in this same run (a placed call whose rectangle is the upper 224 x 224 of a 224 x 448 canvas against the oriented call at 224 x 224: the
     difference is the margin launch); margin: the to_tensor call's own max - min spread.  This is the bar that justifies the fused LDS kernel.
     Also reported, without a bar: HUE alone, GAUSSIAN_BLUR at radius 0.5 and 8, the full recipe.
 (b) wall clock around a synchronise: the augmented call with the full recipe - brightness, contrast, color, hue, gaussian_blur, solarize with
     parameters per sample - is at least 10 x below the host way - to_tensor "uint8" NHWC, tensor_to_host, the Pillow calls per sample, upload of the
     8-bit result (the host way is not even normalised) -, and the two 8-bit results are equal bit for bit (asserted).
Each reports HELD or REFUTED with the numbers.
usage: python tools/measure_augment_output.py [report.txt] [--rehearse], from the repository root after build(); --rehearse runs two small stills once
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

say("expectation (a): to_tensor_augmented with a one-step GAUSSIAN_BLUR chain of radius 2 <= to_tensor + six dense passes over the intermediate (each reads and writes it) at k_canvas_margin's rate of this run + to_tensor's max - min spread")
say("expectation (b): to_tensor_augmented with the full recipe, wall clock around a synchronise, is at least 10 x below to_tensor uint8 + tensor_to_host + the Pillow calls per sample + upload; 8-bit results bit-equal")
say("")

import torch
if not torch.cuda.is_available():
    say("not measured: torch sees no GPU (the events and the output tensors are torch's)")
    sys.exit(1)
try:
    from PIL import Image, ImageEnhance, ImageFilter, ImageOps
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
RESIZE = decoder.SCALE_BILINEAR
kw = dict(dtype="float16", layout="NCHW", mean=MEAN, std=STD, filter=RESIZE)
factors = rng.uniform(0.6, 1.4, (n, 3))
shifts = [decoder.hue_shift(float(f)) for f in rng.uniform(-0.1, 0.1, n)]
radii = rng.uniform(0.1, 2.0, n)
CHAINS = {"HUE": [[("hue", d_)] for d_ in shifts],
          "BLUR0.5": [[("gaussian_blur", 0.5)] for _ in range(n)],
          "BLUR2": [[("gaussian_blur", 2.0)] for _ in range(n)],
          "BLUR8": [[("gaussian_blur", 8.0)] for _ in range(n)],
          "RECIPE": [[("brightness", float(f[0])), ("contrast", float(f[1])), ("color", float(f[2])), ("hue", shifts[e]), ("gaussian_blur", float(radii[e])), ("solarize", 128)]
                     for e, f in enumerate(factors)]}
CHAINS = dict((k, decoder.augment_chains(v, n)) for k, v in CHAINS.items())      # (built once: the calls below time the library, not ctypes)
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    ballast = torch.empty(64 << 20 if REHEARSE else 512 << 20, dtype=torch.uint8, device="cuda")
    plain = torch.empty((n, 3, TS, TS), dtype=torch.float16, device="cuda")
    augmented = torch.empty((n, 3, TS, TS), dtype=torch.float16, device="cuda")
    augmented8 = torch.empty((n, TS, TS, 3), dtype=torch.uint8, device="cuda")
    mid8 = torch.empty((n, TS, TS, 3), dtype=torch.uint8, device="cuda")
    tall = torch.empty((n, 3, 2 * TS, TS), dtype=torch.float16, device="cuda")

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

def unchanged():
    b.to_tensor((TS, TS), entries, out=plain, **kw)
def placed_tall():
    b.to_tensor((TS, 2 * TS), entries, out=tall, places=[(0, 0, TS, TS)] * n, fill=0, **kw)
def oriented():
    b.to_tensor((TS, TS), entries, out=plain, orientations=[0] * n, **kw)
def augmented_call(name):
    return lambda: b.to_tensor_augmented((TS, TS), CHAINS[name], entries, out=augmented, **kw)

ways = [("to_tensor", unchanged), ("placed tall", placed_tall), ("oriented", oriented)] + [(k, augmented_call(k)) for k in CHAINS]
for _, c in ways:
    for _ in range(1 if REHEARSE else 2):
        timed(c)
times = dict((name, []) for name, _ in ways)
for r in range(R):
    for name, c in (ways if r % 2 == 0 else ways[::-1]):
        times[name].append(timed(c))
times = dict((k, np.array(v)) for k, v in times.items())
say("batch: %d generator stills (%d x %d, 8-bit 4:2:0), after run(); %d random-resized-crop windows -> %d x %d float16 NCHW, resize BILINEAR; %d rounds, interleaved "
    "(the order alternates from round to round)" % (N, W, H, n, TS, TS, R))
for name, _ in ways:
    t = times[name]
    say("  %-12s events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f" % (name, t.mean(), np.median(t), t.min(), t.max()))
margin_bytes = n * 3 * TS * TS * 2
margin_ms = times["placed tall"].mean() - times["oriented"].mean()
PASS_BYTES = 2 * n * TS * TS * 3                                     # one box pass as a launch of its own: the intermediate read and written
ok = True
if margin_ms <= 0:
    say("k_canvas_margin, by difference: inside the spread - the dense passes cannot be priced; (a) not decided")
    ok = False
else:
    rate = margin_bytes / (margin_ms * 1e-3)
    PASS_MS = PASS_BYTES / rate * 1e3
    spread = times["to_tensor"].max() - times["to_tensor"].min()
    say("k_canvas_margin, by difference (placed tall - oriented): %.3f ms for %.1f MB of margin -> %.3f TB/s" % (margin_ms, margin_bytes / 1e6, rate / 1e12))
    say("one dense pass, the intermediate read and written: %.1f MB, %.3f ms at that rate; six: %.3f ms; to_tensor's max - min spread: %.3f ms" %
        (PASS_BYTES / 1e6, PASS_MS, 6 * PASS_MS, spread))
    t0, t1 = times["to_tensor"].mean(), times["BLUR2"].mean()
    held = t1 <= t0 + 6 * PASS_MS + spread
    say("(a) BLUR2 %.3f ms against to_tensor %.3f ms + six passes %.3f ms + spread %.3f ms = %.3f ms: %s (the stage costs %.3f ms, %.2f passes)" %
        (t1, t0, 6 * PASS_MS, spread, t0 + 6 * PASS_MS + spread, "HELD" if held else "REFUTED", t1 - t0, (t1 - t0) / PASS_MS))
    ok = ok and held
    for name in ("HUE", "BLUR0.5", "BLUR8", "RECIPE"):
        say("    %-10s the stage costs %.3f ms (%.2f passes)" % (name, times[name].mean() - t0, (times[name].mean() - t0) / PASS_MS))

def pil_recipe(im, e):
    f = [float(v) for v in factors[e]]
    im = ImageEnhance.Color(ImageEnhance.Contrast(ImageEnhance.Brightness(im).enhance(f[0])).enhance(f[1])).enhance(f[2])
    h, s, v = im.convert("HSV").split()
    nh = (np.array(h, np.uint8).astype(np.int32) + shifts[e]).astype(np.uint8)
    im = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
    return ImageOps.solarize(im.filter(ImageFilter.GaussianBlur(float(radii[e]))), 128)

def one_call():
    b.to_tensor_augmented((TS, TS), CHAINS["RECIPE"], entries, out=augmented, **kw)
def one_call8():
    b.to_tensor_augmented((TS, TS), CHAINS["RECIPE"], entries, out=augmented8, dtype="uint8", layout="NHWC", filter=RESIZE)
    return augmented8
def host_way():
    b.to_tensor((TS, TS), entries, out=mid8, dtype="uint8", layout="NHWC", filter=RESIZE)
    host = b.tensor_to_host()
    res = np.stack([np.asarray(pil_recipe(Image.fromarray(host[e]), e)) for e in range(n)])
    return torch.from_numpy(res).to("cuda", non_blocking=False)
say("")
w1 = np.array([wall(one_call)[0] for _ in range(R)])
say("RECIPE: to_tensor_augmented, wall clock around a synchronise: mean %8.3f ms  min %8.3f  max %8.3f" % (w1.mean(), w1.min(), w1.max()))
if Image is None:
    say("(b) not measured: Pillow is not installed")
    ok = False
else:
    hw = []
    for _ in range(1 if REHEARSE else 3):
        ms, res = wall(host_way)
        hw.append(ms)
    hw = np.array(hw)
    _, got8 = wall(one_call8)
    same = bool(torch.equal(res, got8))
    assert same, "the augmented call and Pillow differ"
    far = w1.mean() * 10 <= hw.mean()
    say("RECIPE: host way (to_tensor uint8, tensor_to_host, Pillow per sample, upload), wall clock: mean %8.3f ms  min %8.3f  max %8.3f" % (hw.mean(), hw.min(), hw.max()))
    say("(b) RECIPE: %.3f ms against the host way %.3f ms (%.0f x): %s; the two 8-bit results are equal bit for bit: %s" %
        (w1.mean(), hw.mean(), hw.mean() / w1.mean(), "HELD" if far else "REFUTED (less than 10 x)", same))
    ok = ok and far
s = decoder.augment_stats()
say("")
say("hipdec_augment_stats: %d calls, %d entries, %d launches" % s)
b.free()
say("")
say("done" if ok else "done: AN EXPECTATION WAS MISSED (see above)")
