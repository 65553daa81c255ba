"""Device time of the colour stage (timing slot [5]) for to_rgb_all against to_rgb_scaled_all (480 x 270, NEAREST and BOX) on one batch of 64 generator
4K stills (8-bit 4:2:0), interleaved order, and the host-visible time of RGB -> pinned host, full size against scaled."""
import ctypes as C, glob, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import libheif_amd
from libheif_amd import decoder
from libheif_amd._capi import check

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")   # usage: python tools/measure_scaled_output.py [report.txt], from the repository root after build()
def say(s):
    print(s); out.write(s + "\n"); out.flush()

files = sorted(glob.glob("build/streams/s_3840x2160_*.hevc"))[:64]
assert len(files) == 64, len(files)
streams = [open(f, "rb").read() for f in files]
lib = libheif_amd.load_library()
assert lib.hipdec_init(0) == 0
b = decoder.Batch(streams)
d = b.info(0)
assert (d["width"], d["height"], d["bit_depth_luma"], d["chroma_format_idc"]) == (3840, 2160, 8, 1), d
b.run(); b.status()
b.alloc_rgb(10)
OW, OH = 480, 270
b.alloc_rgb_scaled((OW, OH), 10)
N = 64
px = 3840 * 2160 * N

def colour_us(call):
    call(); b.status()
    return b.slot_kernel_timing_us(0)["colour"]

calls = [("to_rgb_all", lambda: b.to_rgb_all()), ("to_rgb_scaled_all NEAREST", lambda: b.to_rgb_scaled_all(decoder.SCALE_NEAREST)),
         ("to_rgb_scaled_all BOX", lambda: b.to_rgb_scaled_all(decoder.SCALE_BOX))]
for _, c in calls:      # warm-up: code objects, parameter uploads
    for _ in range(2):
        colour_us(c)
R = 12
t = {n: [] for n, _ in calls}
for r in range(R):
    for n, c in calls:
        t[n].append(colour_us(c))
say("batch: 64 generator 4K stills (3840 x 2160, 8-bit 4:2:0), after run(); device time of the colour stage (timing slot [5]), %d calls each, interleaved" % R)
moved = {"to_rgb_all": px * 4.5, "to_rgb_scaled_all NEAREST": OW * OH * N * (3 + 1.5), "to_rgb_scaled_all BOX": px * 1.5 + OW * OH * N * 3}
for n, _ in calls:
    a = np.array(t[n])
    say("%-28s mean %9.1f us  median %9.1f  min %9.1f  max %9.1f   algorithmic bytes %7.1f MB -> %6.2f TB/s at the mean (%4.1f %% of 8 TB/s)" %
        (n, a.mean(), np.median(a), a.min(), a.max(), moved[n] / 1e6, moved[n] / a.mean() / 1e6, moved[n] / a.mean() / 1e6 / 8 * 100))
say("BOX / to_rgb_all device time: %.3f" % (np.mean(t["to_rgb_scaled_all BOX"]) / np.mean(t["to_rgb_all"])))

# host-visible: colour stage + copies of all 64 results into pinned host memory, wall clock
pinned = "pinned (torch)"
try:
    import torch
    full_host = torch.empty(N * 3840 * 2160 * 3, dtype=torch.uint8).pin_memory()
    small_host = torch.empty(N * OW * OH * 3, dtype=torch.uint8).pin_memory()
    fp, sp = full_host.data_ptr(), small_host.data_ptr()
except Exception as e:   # pageable then, and say so
    pinned = "PAGEABLE (no pinned allocation: %s)" % e
    full_host = np.empty(N * 3840 * 2160 * 3, np.uint8); small_host = np.empty(N * OW * OH * 3, np.uint8)
    fp, sp = full_host.ctypes.data, small_host.ctypes.data

def full_to_host():
    b.to_rgb_all()
    nb = 3840 * 2160 * 3
    for i, (buf, _, _) in enumerate(b._rgb):
        check(lib.hipdec_memcpy_d2h(fp + i * nb, buf.ptr, nb))

def scaled_to_host():
    b.to_rgb_scaled_all(decoder.SCALE_BOX)
    nb = OW * OH * 3
    for i, (buf, _, _) in enumerate(b._srgb):
        check(lib.hipdec_memcpy_d2h(sp + i * nb, buf.ptr, nb))

res = {"full": [], "scaled": []}
for f in (full_to_host, scaled_to_host):
    f(); b.status()
for r in range(10):
    for n, f in (("full", full_to_host), ("scaled", scaled_to_host)):
        b.status()
        t0 = time.perf_counter(); f(); b.status(); res[n].append((time.perf_counter() - t0) * 1e3)
say("host-visible, colour stage + 64 device-to-host copies, host memory %s, 10 calls each, interleaved:" % pinned)
say("  full RGB24 (64 x 24.9 MB)        mean %8.2f ms  min %8.2f" % (np.mean(res["full"]), np.min(res["full"])))
say("  BOX 480 x 270 RGB24 (64 x 389 KB) mean %8.2f ms  min %8.2f" % (np.mean(res["scaled"]), np.min(res["scaled"])))
b.free()
say("done")
