"""Clip output (hipdec_clips_*, include/heif_hipdec.h) on 16 generator tracks of 1280 x 720 with 32 samples each (IBBP, 8-bit 4:2:0): 64 clips of T = 16
frames (four per track, each with its own window and flip) to 224 x 224 float16, and the same clips as 448 x 448 token sequences with P = 14, m = 2,
Tp = 2.  All on one build, 12 rounds per figure.

Expectations, stated before the run and reported as HELD or REFUTED with the numbers:
 (a) N C T H W with BOX through the strided box kernel (k_clip_box) is not slower than the same entries through k_oriented_box (the development switch
     HIPDEC_CLIP_NO_STRIDED_BOX, read once per process: the two routes run in child processes of 6 rounds each, started in turn - strided, oriented,
     strided, oriented).  Device time between two events on one stream around the call.  Accepted when the strided mean is at most the oriented mean plus
     the oriented route's max - min spread.
 (b) One Clips object - create, run, ONE to_tensor call - against the way a host has today: 16 HipDecoder objects side by side (one thread each), every
     output picture through hipdec_decoder_device_plane + hipdec_image_to_tensor once per clip that sampled it.  Wall clock around a synchronise, N T C H W
     (the layout today's way can write); the two tensors must be equal bit for bit.  Expected: the clip way is faster.
 (c) Clips create + run + status against those 16 decoder objects playing the same samples (no tensors), frames per second.  Expected: not slower.
Also reported: the token call (device time, slot [5]) and the dense call per filter.

usage, from the repository root after build():
  python tools/measure_clip_output.py --encode             the tracks into build/streams/clip_tracks.pickle (CPU only; minutes)
  python tools/measure_clip_output.py [report.txt]         the measurement (needs the tracks)
  python tools/measure_clip_output.py [report.txt] --rehearse     two small tracks once through every call (the numbers mean nothing)"""
import os, pickle, subprocess, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np

args = [a for a in sys.argv[1:] if not a.startswith("--")]
REHEARSE = "--rehearse" in sys.argv
CHILD = next((a.split("=")[1] for a in sys.argv if a.startswith("--child=")), None)
CACHE = os.path.join(ROOT, "build", "streams", "clip_tracks_small.pickle" if REHEARSE else "clip_tracks.pickle")
W, H, TRACKS, SAMPLES, T, CLIPS_PER_TRACK, OUT, TOK, R = (200, 136, 2, 8, 4, 2, 32, 56, 1) if REHEARSE else (1280, 720, 16, 32, 16, 4, 224, 448, 12)
P, M, TP = 14, 2, 2


def encode_tracks():
    from oracle import pyoracle as orc
    from test_inter_oracle import make_frames
    tracks = []
    for t in range(TRACKS):
        aus = orc.encode_sequence(make_frames(W, H, SAMPLES, seed=5 + t), qp=27, global_mv_x=-8, global_mv_y=-4, inter_skip_pct=30, b_frames=2, inter_num_refs=2,
                                  temporal_mvp=1, seed=t)
        tracks.append([bytes(a) for a in aus])
        print("track %d: %d samples, %.0f KB" % (t, len(aus), sum(len(a) for a in aus) / 1e3), flush=True)
    os.makedirs(os.path.dirname(CACHE), exist_ok=True)
    with open(CACHE, "wb") as f:
        pickle.dump(tracks, f)
    return tracks


if "--encode" in sys.argv:
    encode_tracks()
    sys.exit(0)
tracks = pickle.load(open(CACHE, "rb")) if os.path.exists(CACHE) else (encode_tracks() if REHEARSE else None)
assert tracks is not None, "no tracks: run with --encode first"

# the workload: CLIPS_PER_TRACK clips per track, windows at odd offsets with aspect ratios around the picture's, every other one flipped, uniform sampling
rng = np.random.default_rng(11)
entries, frames = [], []
from libheif_amd import decoder
for t in range(TRACKS):
    for k in range(CLIPS_PER_TRACK):
        ww = int(W * rng.uniform(0.5, 0.95)); wh = int(H * rng.uniform(0.5, 0.95))
        entries.append((t, int(rng.integers(0, W - ww)) | 1, int(rng.integers(0, H - wh)) | 1, ww - 1, wh - 1, k & 1))
        frames.append(decoder.uniform_frames(SAMPLES, T, stride=1 + (k & 1), start=k))
N = len(entries)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
KW = dict(dtype="float16", mean=MEAN, std=STD)


def device_rounds(rounds):
    """per round: device ms between two events around the N C T H W BOX call; torch tensors on one torch stream, as the sibling tools measure"""
    import torch
    c = decoder.Clips(tracks)
    c.run(); c.status()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ballast = torch.empty(64 << 20 if REHEARSE else 512 << 20, dtype=torch.uint8, device="cuda")
        out = torch.empty((N, 3, T, OUT, OUT), dtype=torch.float16, device="cuda")

    def timed(call):
        with torch.cuda.stream(side):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(8):
                ballast.zero_()                                      # the device is busy while the host prepares and enqueues the call
            e0.record(side); call(); e1.record(side)
        side.synchronize(); c.status()
        return e0.elapsed_time(e1), c.batch.slot_kernel_timing_us(0)["colour"]
    res = {}
    toks_out = {}
    offsets, tokens, total = decoder.clip_packed_layout([(TOK, TOK)] * N, T, P, M, TP)
    with torch.cuda.stream(side):
        toks_out["t"] = torch.empty((total,), dtype=torch.float16, device="cuda")
    calls = {"CTHW BOX": lambda: c.to_tensor((OUT, OUT), T, entries, frames, order="CTHW", filter=decoder.SCALE_BOX, out=out, **KW),
             "CTHW NEAREST": lambda: c.to_tensor((OUT, OUT), T, entries, frames, order="CTHW", filter=decoder.SCALE_NEAREST, out=out, **KW),
             "CTHW BICUBIC": lambda: c.to_tensor((OUT, OUT), T, entries, frames, order="CTHW", filter=decoder.SCALE_BICUBIC, out=out, **KW),
             "tokens BOX": lambda: c.to_tokens([(TOK, TOK)] * N, T, entries, frames, P, merge=M, temporal_patch=TP, filter=decoder.SCALE_BOX, offsets=offsets,
                                               out=toks_out["t"], **KW)}
    for name, call in calls.items():
        timed(call); timed(call)
        res[name] = [timed(call) for _ in range(rounds)]
    res["strided_box_entries"] = decoder.clips_stats()[4]
    c.free()
    return res


if CHILD:
    print("RESULT " + repr(device_rounds(R if REHEARSE else R // 2)), flush=True)
    sys.exit(0)

out = open(args[0] if args else os.devnull, "w")
def say(s):
    print(s, flush=True); out.write(s + "\n"); out.flush()

ok = True
say("tracks: %d x %d samples of %d x %d (IBBP, 8-bit 4:2:0); %d clips of T = %d to %d x %d float16; tokens at %d x %d, P = %d, m = %d, Tp = %d" %
    (TRACKS, SAMPLES, W, H, N, T, OUT, OUT, TOK, TOK, P, M, TP))

# ---- (a): the two routes, child processes in turn (nothing of this process has touched the device yet)
routes = {"strided": {}, "oriented": {}}
for turn in range(1 if REHEARSE else 2):
    for route in ("strided", "oriented"):
        env = dict(os.environ)
        env.pop("HIPDEC_CLIP_NO_STRIDED_BOX", None)
        if route == "oriented":
            env["HIPDEC_CLIP_NO_STRIDED_BOX"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child=" + route] + (["--rehearse"] if REHEARSE else []), cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        assert r.returncode == 0 and line, r.stdout[-3000:]
        got = eval(line[-1][7:])
        for k, v in got.items():
            if isinstance(v, list):
                routes[route].setdefault(k, []).extend(v)
            else:
                routes[route][k] = v
say("")
say("device time between two events on one stream, %d rounds per route (child processes in turn):" % len(routes["strided"]["CTHW BOX"]))
for route in ("strided", "oriented"):
    for name in ("CTHW BOX", "CTHW NEAREST", "CTHW BICUBIC", "tokens BOX"):
        ms = np.array([x[0] for x in routes[route][name]]); us = np.array([x[1] for x in routes[route][name]])
        say("  %-8s %-13s events mean %8.3f ms  median %8.3f  min %8.3f  max %8.3f   slot [5] mean %8.1f us" % (route, name, ms.mean(), np.median(ms), ms.min(), ms.max(), us.mean()))
    say("  %-8s frames through k_clip_box in the child: %d" % (route, routes[route]["strided_box_entries"]))
a = np.array([x[0] for x in routes["strided"]["CTHW BOX"]]); b_ = np.array([x[0] for x in routes["oriented"]["CTHW BOX"]])
held = a.mean() <= b_.mean() + (b_.max() - b_.min())
say("(a) N C T H W BOX: k_clip_box mean %.3f ms, k_oriented_box mean %.3f ms (spread %.3f ms): %s" % (a.mean(), b_.mean(), b_.max() - b_.min(), "HELD" if held else "REFUTED"))
ok = ok and held and routes["oriented"]["strided_box_entries"] == 0 and routes["strided"]["strided_box_entries"] > 0

# ---- (b), (c): this process
import libheif_amd
from libheif_amd._capi import DeviceBuffer, ImageInfo, check
from libheif_amd.color import ColorImage, _nclx_struct
lib = decoder._bind(libheif_amd.load_library())
assert lib.hipdec_init(0) == 0
lib.hipdec_decoder_next_picture.argtypes = [C.c_void_p, C.c_int, C.POINTER(ImageInfo), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
lib.hipdec_decoder_device_plane.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
frame_bytes = 3 * OUT * OUT * 2
today_out = DeviceBuffer(N * T * frame_bytes)
clip_out = DeviceBuffer(N * T * frame_bytes)
sc, bi = decoder.tensor_scale_bias(MEAN, STD)
desc = decoder.tensor_desc((OUT, OUT), "float16", "NCHW", decoder.SCALE_BOX, sc, bi)
# frame f of track t -> [(clip, position)] that sampled it
wanted = [[[] for _ in range(SAMPLES)] for _ in range(TRACKS)]
for e, (ent, fr) in enumerate(zip(entries, frames)):
    for k, f in enumerate(fr):
        wanted[ent[0]][f].append((e, k))


def play(t, tensors, errors):
    """track t the way libheif drives a decoder object; every output picture to the clips that sampled it"""
    try:
        d = decoder.HipDecoder()
        info, have, ud = ImageInfo(), C.c_int(0), C.c_size_t(0)
        got = 0

        def take():
            nonlocal got
            if tensors:
                img = ColorImage()
                img.width, img.height, img.chroma, img.bit_depth, img.on_device = info.width, info.height, 1, info.bit_depth_luma, 1
                for c in range(3):
                    p, st = C.c_void_p(), C.c_size_t()
                    check(lib.hipdec_decoder_device_plane(d._h, c, C.byref(p), C.byref(st)))
                    img.plane[c], img.stride[c] = p.value, st.value
                ns = _nclx_struct((info.colour_primaries, info.transfer_characteristics, info.matrix_coeffs, info.full_range_flag))
                for e, k in wanted[t][got]:
                    arr = decoder.tensor_entries([(0,) + tuple(entries[e][1:])])
                    check(lib.hipdec_image_to_tensor(C.byref(img), C.byref(ns), C.byref(desc), arr, 1, today_out.ptr + (e * T + k) * frame_bytes, frame_bytes, 1))
            got += 1
        for au in tracks[t]:
            d.push_data(au)
            while True:
                check(lib.hipdec_decoder_next_picture(d._h, 0, C.byref(info), C.byref(have), C.byref(ud)))
                if not have.value:
                    break
                take()
        while True:
            check(lib.hipdec_decoder_next_picture(d._h, 1, C.byref(info), C.byref(have), C.byref(ud)))
            if not have.value:
                break
            take()
        d.free()
        assert got == SAMPLES, got
    except Exception as ex:      # (a thread's exception would otherwise be lost)
        errors.append(repr(ex))


def today(tensors):
    errors = []
    th = [threading.Thread(target=play, args=(t, tensors, errors)) for t in range(TRACKS)]
    t0 = time.perf_counter()
    for x in th: x.start()
    for x in th: x.join()
    check(lib.hipdec_stream_synchronize(None))
    assert not errors, errors
    return time.perf_counter() - t0


def clips_way(tensors):
    t0 = time.perf_counter()
    c = decoder.Clips(tracks)
    c.run()
    if tensors:
        c.to_tensor((OUT, OUT), T, entries, frames, order="TCHW", filter=decoder.SCALE_BOX, out=clip_out, **KW)
    c.status()
    check(lib.hipdec_stream_synchronize(None))
    dt = time.perf_counter() - t0
    c.free()
    return dt


for tensors in (True, False):
    today(tensors); clips_way(tensors)                               # warm-up
    t_today, t_clips = [], []
    for r in range(R):
        for way in ((today, clips_way) if r % 2 == 0 else (clips_way, today)):
            (t_today if way is today else t_clips).append(way(tensors))
    t_today, t_clips = np.array(t_today) * 1e3, np.array(t_clips) * 1e3
    say("")
    if tensors:
        same = today_out.to_numpy((N * T * frame_bytes,), np.uint8).tobytes() == clip_out.to_numpy((N * T * frame_bytes,), np.uint8).tobytes()
        say("decode + %d clips (N T C H W, BOX), wall clock around a synchronise, %d interleaved rounds:" % (N, R))
        say("  today: 16 decoder objects, %d x hipdec_image_to_tensor   mean %8.1f ms  median %8.1f  min %8.1f  max %8.1f" % (N * T, t_today.mean(), np.median(t_today), t_today.min(), t_today.max()))
        say("  clips: create + run + ONE to_tensor                      mean %8.1f ms  median %8.1f  min %8.1f  max %8.1f" % (t_clips.mean(), np.median(t_clips), t_clips.min(), t_clips.max()))
        say("  the two tensors are equal bit for bit: %s" % same)
        held = t_clips.mean() <= t_today.mean()
        say("(b) %.1f ms against %.1f ms (%.2f x): %s" % (t_clips.mean(), t_today.mean(), t_today.mean() / t_clips.mean(), "HELD" if held else "REFUTED"))
        ok = ok and held and same
    else:
        n = TRACKS * SAMPLES
        say("decode only, %d pictures, wall clock, %d interleaved rounds:" % (n, R))
        say("  today: 16 decoder objects side by side   mean %8.1f ms  (%7.1f fps)  min %8.1f  max %8.1f" % (t_today.mean(), n / t_today.mean() * 1e3, t_today.min(), t_today.max()))
        say("  Clips: create + run + status             mean %8.1f ms  (%7.1f fps)  min %8.1f  max %8.1f" % (t_clips.mean(), n / t_clips.mean() * 1e3, t_clips.min(), t_clips.max()))
        held = t_clips.mean() <= t_today.mean() + (t_today.max() - t_today.min())
        say("(c) %.1f fps against %.1f fps: %s" % (n / t_clips.mean() * 1e3, n / t_today.mean() * 1e3, "HELD" if held else "REFUTED"))
        ok = ok and held
say("done" if ok else "done: AN EXPECTATION WAS MISSED (see above)")
