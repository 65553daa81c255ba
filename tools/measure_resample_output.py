"""The Pillow-exact filters (SCALE_BILINEAR / SCALE_BICUBIC, k_resample) against BOX on the same build and against the two-step way a user has without
them, on one batch of 64 generator 4K stills (8-bit 4:2:0), all in one process, interleaved order.  The two workloads of tools/measure_oriented_output.py:
 thumbnails  64 stills -> 480 x 270 RGB24;
 samples     256 entries (four half-area windows per still) -> 224 x 224 float16 NCHW.
Device time of the colour stage (timing slot [5]) of: BOX (the yardstick, with its max - min spread over the rounds), BILINEAR and BICUBIC with
orientation codes 0 and 1 (code 1 at the swapped size, so the same source pixels are read).  Nothing is gated: the cost over BOX is the extra taps.
The host share of a call is its wall clock until complete minus that device time: it holds the table computation and the upload.  It is reported where
deduplication takes effect (the thumbnails and the four fixed windows share two tables per call) and where it does not (random-resized-crop windows,
drawn anew every round: up to 512 tables, uploaded every time).
Where torch sees the GPU, the two-step way: to_tensor NEAREST uint8 at the window's own size (a copy of the window), then
torch.nn.functional.interpolate(mode="bilinear" / "bicubic", antialias=True) - wall clock until complete, beside the fused call timed the same way.  THAT
PATH IS NOT BIT-EQUAL TO PILLOW (float arithmetic, no 8-bit intermediate); it is what a user has today.  Expected: the fused call is below it at both shapes;
a shape that misses is reported as such.
usage: python tools/measure_resample_output.py [report.txt] [--rehearse], from the repository root after build(); --rehearse runs two small stills once
through every call (no 4K streams needed, the numbers mean nothing)."""
import glob, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import libheif_amd
from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer

args = [a for a in sys.argv[1:] if not a.startswith("--")]
REHEARSE = "--rehearse" in sys.argv
out = open(args[0] if args else os.devnull, "w")
def say(s):
    print(s); out.write(s + "\n"); out.flush()

if REHEARSE:
    from oracle import pyoracle as orc
    W, H, N, OW, OH, TS, R = 200, 136, 2, 50, 34, 24, 1
    streams = [orc.encode(orc.synth_image(W, H, 8, 1, seed=3 + i), bit_depth=8) for i in range(N)]
else:
    W, H, N, OW, OH, TS, R = 3840, 2160, 64, 480, 270, 224, 12
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
RW, RH = int(W / np.sqrt(2)), int(H / np.sqrt(2))
ENTRIES = [(i, (W - RW) * k // 3, (H - RH) * k // 3, RW, RH, 0) for i in range(N) for k in range(4)]      # four half-area windows per still, odd offsets among them
NE = len(ENTRIES)
FILTERS = (("BOX", decoder.SCALE_BOX), ("BILINEAR", decoder.SCALE_BILINEAR), ("BICUBIC", decoder.SCALE_BICUBIC))
rng = np.random.default_rng(7)

try:
    import torch
    assert torch.cuda.is_available()
except Exception:
    torch = None

def timed(call):
    """(device time of the colour stage in us, wall clock until complete in ms)"""
    t0 = time.perf_counter(); call(); b.status()
    wall = (time.perf_counter() - t0) * 1e3
    return b.slot_kernel_timing_us(0)["colour"], wall

def rgb_setter(sizes):
    b.alloc_rgb_scaled(sizes, 10)
    return b._srgb, b._srgb_w, b._srgb_h, b._srgb_ptrs, b._srgb_strides
def use(state):
    b._srgb, b._srgb_w, b._srgb_h, b._srgb_ptrs, b._srgb_strides = state

landscape, portrait = rgb_setter((OW, OH)), rgb_setter((OH, OW))
f16 = DeviceBuffer(NE * TS * TS * 6)
kw = dict(dtype="float16", layout="NCHW", mean=MEAN, std=STD)

def rgb(state, filt, codes):
    use(state); b.to_rgb_scaled_all(filt, orientations=codes)

calls = []      # (workload, name, call)
for fname, filt in FILTERS:
    calls.append(("thumbnails", "%s code 0" % fname, lambda filt=filt: rgb(landscape, filt, None)))
    calls.append(("samples", "%s code 0" % fname, lambda filt=filt: b.to_tensor((TS, TS), ENTRIES, out=f16, filter=filt, **kw)))
    if filt != decoder.SCALE_BOX:
        calls.append(("thumbnails", "%s code 1" % fname, lambda filt=filt: rgb(portrait, filt, [1] * N)))
        calls.append(("samples", "%s code 1" % fname, lambda filt=filt: b.to_tensor((TS, TS), ENTRIES, out=f16, filter=filt, orientations=[1] * NE, **kw)))
        def random_windows(filt=filt):
            e = decoder.random_resized_crop_entries(rng, [(W, H)] * NE, items=[i // 4 for i in range(NE)])
            b.to_tensor((TS, TS), e, out=f16, filter=filt, **kw)
        calls.append(("samples", "%s code 0, random-resized-crop windows (no table is shared)" % fname, random_windows))

for _, _, c in calls:
    for _ in range(1 if REHEARSE else 2):
        timed(c)
dev = {(wl, n): [] for wl, n, _ in calls}
wall = {(wl, n): [] for wl, n, _ in calls}
for r in range(R):
    for wl, n, c in calls:
        us, ms = timed(c)
        dev[(wl, n)].append(us); wall[(wl, n)].append(ms)

say("batch: %d generator stills (%d x %d, 8-bit 4:2:0), after run(); %d rounds, interleaved; device time = the colour stage (timing slot [5]);" % (N, W, H, R))
say("host share = wall clock of the call until complete - device time (table computation and upload are in it)")
for wl, title in (("thumbnails", "thumbnails: %d stills -> %d x %d RGB24 (code 1: %d x %d)" % (N, OW, OH, OH, OW)),
                  ("samples", "samples: %d windows of %d x %d -> %d x %d float16 NCHW" % (NE, RW, RH, TS, TS))):
    say("")
    say(title)
    box = np.array(dev[(wl, "BOX code 0")])
    for (w2, n), v in dev.items():
        if w2 != wl:
            continue
        a, ww = np.array(v), np.array(wall[(w2, n)])
        say("  %-64s device mean %9.1f us  median %9.1f  min %9.1f  max %9.1f  = %5.2f x BOX   host share mean %7.3f ms" %
            (n, a.mean(), np.median(a), a.min(), a.max(), a.mean() / box.mean(), float(np.mean(ww - a / 1e3))))
    say("  BOX spread (max - min): %.1f us" % (box.max() - box.min()))

ok = True
if torch is not None:
    import torch.nn.functional as F
    say("")
    say("the two-step way (NOT bit-equal to Pillow: float arithmetic, no 8-bit intermediate), wall clock until complete, beside the fused call timed the same way")
    shapes = [("thumbnails", None, N, (W, H), (OW, OH)), ("samples", ENTRIES, NE, (RW, RH), (TS, TS))]
    for wl, entries, n, (sw, sh), (ow, oh) in shapes:
      try:
          src = torch.empty((n, 3, sh, sw), dtype=torch.uint8, device="cuda")
          dst = torch.empty((n, 3, oh, ow), dtype=torch.float16, device="cuda")
          keep = {}
          for mode, filt in (("bilinear", decoder.SCALE_BILINEAR), ("bicubic", decoder.SCALE_BICUBIC)):
              def two_step():
                  b.to_tensor((sw, sh), entries, dtype="uint8", layout="NCHW", filter=decoder.SCALE_NEAREST, out=src)
                  b.status()
                  keep["r"] = F.interpolate(src.float(), size=(oh, ow), mode=mode, antialias=True, align_corners=False)
                  torch.cuda.synchronize()
              def fused():
                  b.to_tensor((ow, oh), entries, dtype="float16", layout="NCHW", scale=1.0, bias=0.0, filter=filt, out=dst)
                  b.status()
                  torch.cuda.synchronize()
              t = {"two-step": [], "fused": []}
              for _ in range(1 if REHEARSE else 2):
                  timed(two_step); timed(fused)
              for r in range(max(1, R // 2)):
                  t["two-step"].append(timed(two_step)[1]); t["fused"].append(timed(fused)[1])
              a, f = np.array(t["two-step"]), np.array(t["fused"])
              good = f.mean() < a.mean()
              ok = ok and good
              diff = (keep["r"].clamp(0, 255).round() - dst.float()).abs()
              say("  %-10s %-8s two-step wall mean %9.3f ms (min %9.3f)   fused wall mean %8.3f ms (min %8.3f): %s; largest difference of the two results %.0f of 255" %
                  (wl, mode, a.mean(), a.min(), f.mean(), f.min(), "fused is below" if good else "FUSED IS NOT BELOW", float(diff.max())))
          del src, dst, keep
          torch.cuda.empty_cache()
      except Exception as e:      # (the report of the device times above stands on its own)
        ok = False
        say("  %s: the two-step comparison failed: %r" % (wl, e))
else:
    say("")
    say("two-step way with torch.nn.functional.interpolate: not measured (torch sees no GPU)")
b.free()
say("")
say("done" if ok else "done: AN EXPECTATION WAS MISSED (see above)")
