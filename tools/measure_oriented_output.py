"""Oriented output against the unoriented calls it is defined by and against the two-step way a host has without it, on one batch of 64 generator 4K stills
(8-bit 4:2:0), all in one process, interleaved order, for both filters.  Two workloads:
 thumbnails  64 stills -> 480 x 270 RGB24 (the shape of profiles/scaled_output.txt);
 samples     256 entries (four windows per still) -> 224 x 224 float16 NCHW.
Three forms on the same build, device time of the colour stage (timing slot [5]):
 (a) the unoriented call (to_rgb_scaled_all / to_tensor): the yardstick; its max - min over the rounds of this run is the spread the rest is judged by;
 (b) code 2 (half turn: rows stay rows).  Expected: mean within mean of (a) + that spread;
 (c) code 1 and code 7 (quarter turns) at the swapped size, so the same source pixels are read.
The two-step way, as the comparison for (c), wall clock until the result is complete (the rotation pass has no timing slot; (c) is timed the same way beside
it): the unoriented call followed by a rotation of its result - hipdec_plane_rotate_ccw per channel plane of a uint8 NCHW tensor for the thumbnails,
torch.rot90(...).contiguous() for the float tensor.  Expected: (c) below the two-step time at every shape.
A shape that misses an expectation is reported as such.  usage: python tools/measure_oriented_output.py [report.txt] [--rehearse], from the repository root
after build(); --rehearse runs two small stills once through every call (no 4K streams needed, the numbers mean nothing)."""
import ctypes as C, glob, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import libheif_amd
from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer, check

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
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
lib.hipdec_plane_rotate_ccw.argtypes = [vp, sz, ci, ci, ci, ci, vp, sz, vp]
b = decoder.Batch(streams)
d = b.info(0)
assert (d["width"], d["height"], d["bit_depth_luma"], d["chroma_format_idc"]) == (W, H, 8, 1), d
b.run(); b.status()
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RW, RH = int(W / np.sqrt(2)), int(H / np.sqrt(2))
ENTRIES = [(i, (W - RW) * k // 3, (H - RH) * k // 3, RW, RH, 0) for i in range(N) for k in range(4)]      # four half-area windows per still, odd offsets among them
NE = len(ENTRIES)
FILTERS = (("BOX", decoder.SCALE_BOX), ("NEAREST", decoder.SCALE_NEAREST))

try:
    import torch
    assert torch.cuda.is_available()
except Exception:
    torch = None

def colour_us(call):
    call(); b.status()
    return b.slot_kernel_timing_us(0)["colour"]

def wall_ms(call):
    t0 = time.perf_counter(); call(); b.status()
    return (time.perf_counter() - t0) * 1e3

def rgb_setter(sizes):
    """the buffers of alloc_rgb_scaled for one size, kept so that the forms can alternate without allocating"""
    b.alloc_rgb_scaled(sizes, 10)
    return b._srgb, b._srgb_w, b._srgb_h, b._srgb_ptrs, b._srgb_strides
def use(state):
    b._srgb, b._srgb_w, b._srgb_h, b._srgb_ptrs, b._srgb_strides = state

landscape, portrait = rgb_setter((OW, OH)), rgb_setter((OH, OW))
u8_land, u8_port = DeviceBuffer(N * OW * OH * 3), DeviceBuffer(N * OW * OH * 3)
u8_rot = DeviceBuffer(N * OW * OH * 3)
f16_a, f16_b = DeviceBuffer(NE * TS * TS * 6), DeviceBuffer(NE * TS * TS * 6)

def rotate_planes():
    for k in range(N * 3):      # every channel plane of the uint8 NCHW tensor: OW x OH -> OH x OW
        check(lib.hipdec_plane_rotate_ccw(u8_land.ptr + k * OW * OH, OW, OW, OH, 1, 90, u8_rot.ptr + k * OW * OH, OH, None))
    check(lib.hipdec_stream_synchronize(None))

ok = True
say("batch: %d generator stills (%d x %d, 8-bit 4:2:0), after run(); %d rounds, interleaved; device time = the colour stage (timing slot [5])" % (N, W, H, R))
for fname, filt in FILTERS:
    in_bytes = W * H * N * 1.5 if filt == decoder.SCALE_BOX else OW * OH * N * 1.5
    def rgb(state, codes):
        use(state); b.to_rgb_scaled_all(filt, orientations=codes)
    dev = [("(a) to_rgb_scaled_all %dx%d" % (OW, OH), lambda: rgb(landscape, None)),
           ("(b) oriented code 2 %dx%d" % (OW, OH), lambda: rgb(landscape, [2] * N)),
           ("(c) oriented code 1 %dx%d" % (OH, OW), lambda: rgb(portrait, [1] * N)),
           ("(c) oriented code 7 %dx%d" % (OH, OW), lambda: rgb(portrait, [7] * N)),
           ("(c) oriented code 1 uint8 NCHW %dx%d" % (OH, OW),
            lambda: b.to_tensor((OH, OW), None, dtype="uint8", layout="NCHW", filter=filt, out=u8_port, orientations=[1] * N))]
    two_step = lambda: (b.to_tensor((OW, OH), None, dtype="uint8", layout="NCHW", filter=filt, out=u8_land), b.status(), rotate_planes())
    wall = [("two-step: to_tensor uint8 NCHW %dx%d, then %d x hipdec_plane_rotate_ccw" % (OW, OH, 3 * N), two_step), ("(c) oriented code 1 uint8 NCHW, one call", dev[4][1])]
    for _, c in dev + wall:
        for _ in range(1 if REHEARSE else 2):
            colour_us(c)
    t = {n: [] for n, _ in dev}
    w = {n: [] for n, _ in wall}
    for r in range(R):
        for n, c in dev:
            t[n].append(colour_us(c))
        for n, c in wall:
            w[n].append(wall_ms(c))
    say("")
    say("thumbnails, %s: %d stills -> %d x %d RGB24" % (fname, N, OW, OH))
    for n, _ in dev:
        a = np.array(t[n])
        moved = OW * OH * N * 3
        say("  %-46s mean %8.1f us  median %8.1f  min %8.1f  max %8.1f   write %5.1f MB -> %5.3f TB/s  (read %6.1f MB)" %
            (n, a.mean(), np.median(a), a.min(), a.max(), moved / 1e6, moved / a.mean() / 1e6, in_bytes / 1e6))
    ya = np.array(t[dev[0][0]])
    spread = ya.max() - ya.min()
    mb = float(np.mean(t[dev[1][0]]))
    good = mb <= ya.mean() + spread
    ok = ok and good
    say("  (b) against (a): %.1f us against %.1f + spread %.1f = %.1f: %s" % (mb, ya.mean(), spread, ya.mean() + spread, "within" if good else "ABOVE THE SPREAD"))
    for n, _ in wall:
        a = np.array(w[n])
        say("  %-78s wall mean %8.3f ms  min %8.3f  max %8.3f" % (n, a.mean(), a.min(), a.max()))
    good = np.mean(w[wall[1][0]]) < np.mean(w[wall[0][0]])
    ok = ok and good
    say("  (c) against the two-step way: %s" % ("below" if good else "NOT BELOW"))
    same = np.array_equal(u8_rot.to_numpy((N * 3, OW, OH), np.uint8), u8_port.to_numpy((N * 3, OW, OH), np.uint8))
    say("  the two results are equal byte for byte: %s" % same)
    ok = ok and same

    # samples
    kw = dict(dtype="float16", layout="NCHW", mean=MEAN, std=STD, filter=filt)
    dev = [("(a) to_tensor %d entries f16 NCHW %dx%d" % (NE, TS, TS), lambda: b.to_tensor((TS, TS), ENTRIES, out=f16_a, **kw)),
           ("(b) oriented code 2", lambda: b.to_tensor((TS, TS), ENTRIES, out=f16_b, orientations=[2] * NE, **kw)),
           ("(c) oriented code 1", lambda: b.to_tensor((TS, TS), ENTRIES, out=f16_b, orientations=[1] * NE, **kw)),
           ("(c) oriented code 7", lambda: b.to_tensor((TS, TS), ENTRIES, out=f16_b, orientations=[7] * NE, **kw))]
    wall = []
    if torch is not None:
        ta = torch.empty((NE, 3, TS, TS), dtype=torch.float16, device="cuda")
        tb = torch.empty((NE, 3, TS, TS), dtype=torch.float16, device="cuda")
        keep = {}
        def two_step_torch():
            b.to_tensor((TS, TS), ENTRIES, out=ta, **kw)
            b.status()
            keep["r"] = torch.rot90(ta, 1, dims=(2, 3)).contiguous()
            torch.cuda.synchronize()
        def one_call_torch():
            b.to_tensor((TS, TS), ENTRIES, out=tb, orientations=[1] * NE, **kw)
            b.status()
            torch.cuda.synchronize()
        wall = [("two-step: to_tensor, then torch.rot90(t, 1, (2, 3)).contiguous()", two_step_torch), ("(c) oriented code 1 into a torch tensor, one call", one_call_torch)]
    for _, c in dev + wall:
        for _ in range(1 if REHEARSE else 2):
            colour_us(c)
    t = {n: [] for n, _ in dev}
    w = {n: [] for n, _ in wall}
    for r in range(R):
        for n, c in dev:
            t[n].append(colour_us(c))
        for n, c in wall:
            w[n].append(wall_ms(c))
    say("samples, %s: %d windows of %d x %d -> %d x %d float16 NCHW" % (fname, NE, RW, RH, TS, TS))
    for n, _ in dev:
        a = np.array(t[n])
        moved = TS * TS * NE * 6
        say("  %-46s mean %8.1f us  median %8.1f  min %8.1f  max %8.1f   write %5.1f MB -> %5.3f TB/s" %
            (n, a.mean(), np.median(a), a.min(), a.max(), moved / 1e6, moved / a.mean() / 1e6))
    ya = np.array(t[dev[0][0]])
    spread = ya.max() - ya.min()
    mb = float(np.mean(t[dev[1][0]]))
    good = mb <= ya.mean() + spread
    ok = ok and good
    say("  (b) against (a): %.1f us against %.1f + spread %.1f = %.1f: %s" % (mb, ya.mean(), spread, ya.mean() + spread, "within" if good else "ABOVE THE SPREAD"))
    if wall:
        for n, _ in wall:
            a = np.array(w[n])
            say("  %-78s wall mean %8.3f ms  min %8.3f  max %8.3f" % (n, a.mean(), a.min(), a.max()))
        good = np.mean(w[wall[1][0]]) < np.mean(w[wall[0][0]])
        ok = ok and good
        say("  (c) against the two-step way: %s" % ("below" if good else "NOT BELOW"))
        same = bool(torch.equal(keep["r"], tb))
        say("  the two results are equal bit for bit: %s" % same)
        ok = ok and same
    else:
        say("  two-step way with torch.rot90: not measured (torch sees no GPU)")
say("")
say("context, not a bar: the album paste kernel writes at 5.3 TB/s (profiles/album.txt); the figures above divide the OUTPUT bytes alone by the time of a kernel that also reads and averages its input")
b.free()
say("done" if ok else "done: AN EXPECTATION WAS MISSED (see above)")
