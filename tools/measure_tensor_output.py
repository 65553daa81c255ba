"""Device time of the colour stage (timing slot [5]) for Batch.to_tensor against the scaled output it is built on, on one batch of 64 generator 4K stills
(8-bit 4:2:0), all in one process, interleaved order:
 (a) to_rgb_scaled_all BOX to 480 x 270: the yardstick, the same read traffic;
 (b) to_tensor of the whole pictures at 480 x 270: uint8 NHWC BOX (byte-identical work to (a)) and float16 NCHW BOX (twice the output bytes);
     accepted when its mean is no more than the mean of (a) plus the max - min spread of (a) in this run;
 (c) to_tensor of a centred half-area window to 224 x 224, float16 NCHW BOX (recorded; half the bytes read);
 (d) the loader's alternative on the same planes: to_rgb_all, then torch crop + interpolate(mode="area") + permute + half + normalise (recorded only:
     torch's area filter is not bit-identical), device and wall time beside (c)."""
import ctypes as C, glob, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import libheif_amd
from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer, check

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")   # usage: python tools/measure_tensor_output.py [report.txt], from the repository root after build()
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
W, H, N = 3840, 2160, 64
OW, OH = 480, 270
b.alloc_rgb_scaled((OW, OH), 10)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RW, RH = int(W / np.sqrt(2)), int(H / np.sqrt(2))                 # the centred half-area window
WINDOW = [decoder.center_crop_entry(i, W, H, RW, RH) for i in range(N)]
buf_u8 = DeviceBuffer(N * OW * OH * 3)
buf_f16 = DeviceBuffer(N * OW * OH * 3 * 2)
buf_224 = DeviceBuffer(N * 224 * 224 * 3 * 2)

def colour_us(call):
    call(); b.status()
    return b.slot_kernel_timing_us(0)["colour"]

calls = [("(a) to_rgb_scaled_all BOX 480x270", lambda: b.to_rgb_scaled_all(decoder.SCALE_BOX), W * H * N * 1.5 + OW * OH * N * 3),
         ("(b) to_tensor u8 NHWC BOX 480x270", lambda: b.to_tensor((OW, OH), None, dtype="uint8", layout="NHWC", out=buf_u8), W * H * N * 1.5 + OW * OH * N * 3),
         ("(b) to_tensor f16 NCHW BOX 480x270", lambda: b.to_tensor((OW, OH), None, dtype="float16", layout="NCHW", mean=MEAN, std=STD, out=buf_f16),
          W * H * N * 1.5 + OW * OH * N * 6),
         ("(c) to_tensor f16 NCHW BOX half-area window -> 224x224", lambda: b.to_tensor((224, 224), WINDOW, dtype="float16", layout="NCHW", mean=MEAN, std=STD, out=buf_224),
          RW * RH * N * 1.5 + 224 * 224 * N * 6),
         ("    to_tensor f16 NCHW NEAREST half-area window -> 224x224",
          lambda: b.to_tensor((224, 224), WINDOW, dtype="float16", layout="NCHW", mean=MEAN, std=STD, filter=decoder.SCALE_NEAREST, out=buf_224), 224 * 224 * N * (1.5 + 6))]
for _, c, _ in calls:      # warm-up: code objects, parameter uploads
    for _ in range(2):
        colour_us(c)
R = 12
t = {n: [] for n, _, _ in calls}
for r in range(R):
    for n, c, _ in calls:
        t[n].append(colour_us(c))
say("batch: 64 generator 4K stills (3840 x 2160, 8-bit 4:2:0), after run(); device time of the colour stage (timing slot [5]), %d calls each, interleaved" % R)
say("window of (c): %d x %d at (%d, %d)" % (RW, RH, WINDOW[0][1], WINDOW[0][2]))
for n, _, moved in calls:
    a = np.array(t[n])
    say("%-58s mean %8.1f us  median %8.1f  min %8.1f  max %8.1f   algorithmic bytes %6.1f MB -> %5.2f TB/s at the mean (%4.1f %% of 8 TB/s)" %
        (n, a.mean(), np.median(a), a.min(), a.max(), moved / 1e6, moved / a.mean() / 1e6, moved / a.mean() / 1e6 / 8 * 100))
ya = np.array(t[calls[0][0]])
bound = ya.mean() + (ya.max() - ya.min())
say("acceptance of (b): mean <= mean of (a) + (max - min) of (a) = %.1f + %.1f = %.1f us" % (ya.mean(), ya.max() - ya.min(), bound))
ok = True
for n, _, _ in calls[1:3]:
    m = float(np.mean(t[n]))
    ok = ok and m <= bound
    say("  %-56s mean %8.1f us: %s" % (n, m, "within" if m <= bound else "ABOVE THE BOUND"))
say("(c) / (b) f16 device time: %.3f (the window holds %.3f of the picture's samples)" % (np.mean(t[calls[3][0]]) / np.mean(t[calls[2][0]]), RW * RH / (W * H)))
same = np.array_equal(buf_u8.to_numpy((N, OH, OW * 3), np.uint8), np.stack([b.rgb_scaled(i) for i in range(N)]))
say("uint8 NHWC tensor of (b) equals the %d buffers of (a) byte for byte: %s" % (N, same))

# (d) the framework path over full-size RGB24
try:
    import torch
    import torch.nn.functional as F
    assert torch.cuda.is_available()
    full = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    b._rgb_chroma = 10
    b._rgb_ptrs = (C.c_void_p * N)(*[full.data_ptr() + i * H * W * 3 for i in range(N)])
    b._rgb_strides = (C.c_size_t * N)(*[W * 3] * N)
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    left, top = WINDOW[0][1], WINDOW[0][2]

    def framework():
        x = full[:, top:top + RH, left:left + RW, :].permute(0, 3, 1, 2).float()
        x = F.interpolate(x, size=(224, 224), mode="area")
        return ((x / 255.0 - mean) / std).half()

    def alt():
        b.to_rgb_all()
        b.status()                      # (the library's stream and torch's are ordered on the host here)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); y = framework(); e1.record()
        torch.cuda.synchronize()
        return b.slot_kernel_timing_us(0)["colour"], e0.elapsed_time(e1) * 1e3, y

    def ours():
        b.to_tensor((224, 224), WINDOW, dtype="float16", layout="NCHW", mean=MEAN, std=STD, out=buf_224)
        b.status()

    for _ in range(2):
        alt(); ours()
    res = {"rgb": [], "torch": [], "alt_wall": [], "ours_wall": []}
    for r in range(10):
        t0 = time.perf_counter(); c_us, f_us, y = alt(); res["alt_wall"].append((time.perf_counter() - t0) * 1e3)
        res["rgb"].append(c_us); res["torch"].append(f_us)
        t0 = time.perf_counter(); ours(); res["ours_wall"].append((time.perf_counter() - t0) * 1e3)
    say("(d) the framework path (torch %s) on the same window, 10 calls each, interleaved with (c):" % torch.__version__)
    say("  to_rgb_all (64 x 24.9 MB RGB24)                        device mean %8.1f us" % np.mean(res["rgb"]))
    say("  crop + interpolate(area) + permute + half + normalise   device mean %8.1f us (torch events)" % np.mean(res["torch"]))
    say("  both, wall clock until the tensor is complete           mean %8.2f ms  min %8.2f" % (np.mean(res["alt_wall"]), np.min(res["alt_wall"])))
    say("  (c) to_tensor, wall clock until the tensor is complete  mean %8.2f ms  min %8.2f" % (np.mean(res["ours_wall"]), np.min(res["ours_wall"])))
    got = torch.from_numpy(buf_224.to_numpy((N, 3, 224, 224), np.float16)).cuda().float()
    say("  largest |difference| between the two tensors: %.4f (torch's area filter is another definition; one 8-bit step is %.4f here)" %
        (float((got - y.float()).abs().max()), 1 / 255 / min(STD)))
except Exception as e:
    say("(d) not measured: %r" % (e,))
b.free()
say("done" if ok else "done: (b) ABOVE THE BOUND")
