"""Recipe tensor output (hipdec_batch_to_tensor_recipe, k_recipe_affine_* beside the photo and augment kernels) on the photo section's workload: one batch
of 64 generator 4K stills (8-bit 4:2:0), 256 random-resized-crop windows (four per still) resized with BILINEAR to 224 x 224, float16 NCHW with the
ImageNet mean / std.  All in one process on one build, 12 interleaved rounds, device time between two events on one torch stream (other work is queued in
front of the first event, so that the launches wait in the queue and the time is the device's).

The recipe: per sample two operations drawn with a fixed seed from the fourteen of torchvision's RandAugment list (Identity, ShearX, ShearY, TranslateX,
TranslateY, Rotate, Brightness, Color, Contrast, Sharpness, Posterize, Solarize, AutoContrast, Equalize) at magnitude bin 9 of 31 with a random sign - the
drawing and the magnitudes are this script's own; the library has no samplers.  One warp filter (BILINEAR) and one fill (black), so that the baseline can
express it.

Expectation, written into the report before anything is measured: ONE recipe call is not slower than the three-pass way the library offered before it -
to_tensor uint8 NHWC, tensor_warp with identity maps where a sample has no geometric first step, tensor_photo, tensor_warp again into the float tensor -,
accepting up to the baseline's mean plus its own max - min spread; the two results are equal bit for bit (asserted).  The baseline's calls are not the code
under test.  Reported beside it, without a bar: the recipe with a filter drawn per operation (BILINEAR or BICUBIC) and a dataset-mean fill, which the
three-pass way cannot express, and the launch count of each.
usage: python tools/measure_recipe_output.py [report.txt] [--rehearse], from the repository root after build(); --rehearse runs two small stills once through
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

say("expectation: one to_tensor_recipe call (two drawn RandAugment operations per sample, BILINEAR, black fill) <= the three-pass way (to_tensor uint8 NHWC, "
    "tensor_warp, tensor_photo, tensor_warp) mean + its own max - min spread; results bit-equal")
say("")

import torch
if not torch.cuda.is_available():
    say("not measured: torch sees no GPU (the events and the tensors are torch's)")
    sys.exit(1)

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
MEAN_FILL = (124, 116, 104)
rng = np.random.default_rng(2026)
entries = decoder.random_resized_crop_entries(rng, [(W, H)] * (N * PER), items=[i % N for i in range(N * PER)])
n = len(entries)
SIZE = (TS, TS)
RESIZE, BILINEAR, BICUBIC = decoder.SCALE_BILINEAR, decoder.SCALE_BILINEAR, decoder.SCALE_BICUBIC
kw = dict(dtype="float16", layout="NCHW", mean=MEAN, std=STD)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
NAMES = ["Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness", "Posterize", "Solarize",
         "AutoContrast", "Equalize"]
BIN = 9.0 / 30.0

def draw():
    """one operation: ("geo", map) | ("col", name, value) | None (Identity)"""
    name = NAMES[int(rng.integers(0, len(NAMES)))]
    sign = -1.0 if rng.uniform() < 0.5 else 1.0
    if name == "Identity":
        return None
    if name == "ShearX":
        return ("geo", decoder.shear_matrix(sign * 0.3 * BIN, 0.0))
    if name == "ShearY":
        return ("geo", decoder.shear_matrix(0.0, sign * 0.3 * BIN))
    if name == "TranslateX":
        return ("geo", decoder.translate_matrix(sign * int(150.0 / 331.0 * TS * BIN), 0.0))
    if name == "TranslateY":
        return ("geo", decoder.translate_matrix(0.0, sign * int(150.0 / 331.0 * TS * BIN)))
    if name == "Rotate":
        return ("geo", decoder.rotate_matrix(sign * 30.0 * BIN, SIZE))
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        return ("col", name.lower(), 1.0 + sign * 0.9 * BIN)
    if name == "Posterize":
        return ("col", "posterize", 8 - int(BIN * 4))
    if name == "Solarize":
        return ("col", "solarize", 255.0 - 255.0 * BIN)
    return ("col", name.lower(), 0.0)

drawn = [[o for o in (draw(), draw()) if o is not None] for _ in range(n)]

def recipe_chains(per_operation):
    frng = np.random.default_rng(7)
    chains = []
    for ops in drawn:
        ch = []
        for o in ops:
            if o[0] == "geo":
                filt = (BICUBIC if frng.uniform() < 0.5 else BILINEAR) if per_operation else BILINEAR
                ch.append(("affine", o[1], filt, MEAN_FILL if per_operation else 0))
            else:
                ch.append((o[1], o[2]))
        chains.append(ch)
    return chains

# the three-pass way: a geometric FIRST step goes into the first warp, every other geometric step into the second; the colour steps in between
maps1, maps2, photo = [], [], []
for ops in drawn:
    first = ops[0][1] if ops and ops[0][0] == "geo" else IDENTITY
    rest = ops[1:] if ops and ops[0][0] == "geo" else ops
    later = [o[1] for o in rest if o[0] == "geo"]
    cols = [(o[1], o[2]) for o in rest if o[0] == "col"]
    assert len(later) <= 1 and (not later or rest[-1][0] == "geo")          # two drawn steps: colour never follows the second warp
    maps1.append(first); maps2.append(later[0] if later else IDENTITY); photo.append(cols)
kinds = [sum(o[0] == "geo" for o in ops) for ops in drawn]
say("drawn: %d samples; %d with no geometric step, %d with one, %d with two; %d Identity draws" %
    (n, kinds.count(0), kinds.count(1), kinds.count(2), 2 * n - sum(len(o) for o in drawn)))

CH_ONE, CH_PER = recipe_chains(False), recipe_chains(True)
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    ballast = torch.empty(64 << 20 if REHEARSE else 512 << 20, dtype=torch.uint8, device="cuda")
    mid8 = torch.empty((n, TS, TS, 3), dtype=torch.uint8, device="cuda")
    w8 = torch.empty((n, TS, TS, 3), dtype=torch.uint8, device="cuda")
    p8 = torch.empty((n, TS, TS, 3), dtype=torch.uint8, device="cuda")
    base = torch.empty((n, 3, TS, TS), dtype=torch.float16, device="cuda")
    one = torch.empty((n, 3, TS, TS), dtype=torch.float16, device="cuda")
    per = torch.empty((n, 3, TS, TS), dtype=torch.float16, device="cuda")

def timed(call):
    """device ms between two events on `side` around what `call` enqueues"""
    with torch.cuda.stream(side):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(64):
            ballast.zero_()                                          # the device is busy while the host prepares and enqueues the calls
        e0.record(side); call(); e1.record(side)
    side.synchronize(); b.status()
    return e0.elapsed_time(e1)

def three_pass():
    b.to_tensor(SIZE, entries, out=mid8, dtype="uint8", layout="NHWC", filter=RESIZE)
    decoder.tensor_warp(mid8, SIZE, maps1, warp_filter=BILINEAR, fill=0, dtype="uint8", layout="NHWC", out=w8)
    decoder.tensor_photo(w8, photo, dtype="uint8", layout="NHWC", out=p8)
    decoder.tensor_warp(p8, SIZE, maps2, warp_filter=BILINEAR, fill=0, out=base, **kw)
def recipe_one():
    b.to_tensor_recipe(SIZE, CH_ONE, entries, out=one, filter=RESIZE, **kw)
def recipe_per():
    b.to_tensor_recipe(SIZE, CH_PER, entries, out=per, filter=RESIZE, **kw)

def launches_of(call):
    """kernel launches of the stages (the resize launch counted once per to_tensor-like call)"""
    s0 = (decoder.warp_stats()[0], decoder.photo_stats()[2], decoder.recipe_stats()[2])
    timed(call)
    s1 = (decoder.warp_stats()[0], decoder.photo_stats()[2], decoder.recipe_stats()[2])
    return 1 + sum(a - c for a, c in zip(s1, s0))

ways = [("three-pass", three_pass), ("recipe", recipe_one), ("recipe/op", recipe_per)]
counts = dict((name, launches_of(c)) for name, c in ways)
for _, c in ways:
    for _ in range(0 if REHEARSE else 2):
        timed(c)
with torch.cuda.stream(side):
    same = bool(torch.equal(base.view(torch.int16), one.view(torch.int16)))
side.synchronize()
assert same, "the recipe call and the three-pass way differ"
times = dict((name, []) for name, _ in ways)
for r in range(R):
    for name, c in (ways if r % 2 == 0 else ways[::-1]):
        times[name].append(timed(c))
times = dict((k, np.array(v)) for k, v in times.items())
say("batch: %d generator stills (%d x %d, 8-bit 4:2:0), after run(); %d random-resized-crop windows -> %d x %d float16 NCHW, resize BILINEAR; %d rounds, interleaved "
    "(the order alternates from round to round)" % (N, W, H, n, TS, TS, R))
for name, _ in ways:
    t = times[name]
    say("  %-11s events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f   launches %d" % (name, t.mean(), np.median(t), t.min(), t.max(), counts[name]))
t0, t1 = times["three-pass"], times["recipe"]
spread = t0.max() - t0.min()
held = t1.mean() <= t0.mean() + spread
say("recipe %.3f ms against the three-pass way %.3f ms + its spread %.3f ms = %.3f ms: %s; the two float16 tensors are equal bit for bit: %s" %
    (t1.mean(), t0.mean(), spread, t0.mean() + spread, "HELD" if held else "REFUTED", same))
say("without a bar: a filter drawn per operation (BILINEAR or BICUBIC) and the fill %s: %.3f ms, %d launches (the three-pass way cannot express it)" %
    (MEAN_FILL, times["recipe/op"].mean(), counts["recipe/op"]))
say("")
say("hipdec_recipe_stats: %d calls, %d entries, %d launches, %d affine steps" % decoder.recipe_stats())
b.free()
say("")
say("done" if held else "done: THE EXPECTATION WAS MISSED (see above)")
