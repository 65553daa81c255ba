"""K grid photos through ONE Album (one launch set + one paste launch) against the same K photos through K GridDecoderC objects on the same build - what a
host with an album can do without hipdec_album_*.  K = 1, 4, 16; a photo is the S3 shape of tests/test_full_shape_gpu.py: 6 x 8 generator tiles of
1024 x 1024 (8-bit 4:2:0, WPP), output 8064 x 6048 so that the right column and the bottom row are clipped; photo k takes the 48 tiles rotated by k.

All in one process, objects created outside the timed windows, every window a host clock around work that ends in a device synchronisation, the
forms alternating inside each repetition:
  grids, in turn     for every photo: hipdec_grid_decode, hipdec_grid_wait
  grids, enqueued    hipdec_grid_decode of every photo, then hipdec_grid_wait of every photo
  album              hipdec_album_run, hipdec_album_status
and beside them the device time of the paste launch (HIP events around it) and the per-kernel device times of the same K x 48 tiles as a plain Batch
(the album's launch set).  usage, from the repository root after build():  python tools/measure_album.py [report.txt]"""
import os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import libheif_amd
from libheif_amd import decoder
from libheif_amd.grid import GridDecoderC, GridLayout
from tools import streamgen

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")
def say(s):
    print(s); out.write(s + "\n"); out.flush()

ROWS, COLS, TW, TH, OW, OH = 6, 8, 1024, 1024, 8064, 6048
VUI = dict(vui_primaries=1, vui_transfer=13, vui_matrix=6, vui_full_range=1)
tiles = streamgen.make_streams([(TW, TH, 2 + t, 8, VUI) for t in range(ROWS * COLS)])
lib = libheif_amd.load_library()
assert lib.hipdec_init(0) == 0, lib.hipdec_last_error()
say("command: python tools/measure_album.py %s" % " ".join(sys.argv[1:]))
say("photo: %d x %d tiles of %d x %d (8-bit 4:2:0, %.2f MB coded), output %d x %d = %.1f Mpixel; R repetitions, forms alternating; host clock around run .. synchronise"
    % (ROWS, COLS, TW, TH, sum(len(t) for t in tiles) / 1e6, OW, OH, OW * OH / 1e6))

def clock(f):
    t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3

for K in (1, 4, 16):
    photos = [tiles[k % len(tiles):] + tiles[:k % len(tiles)] for k in range(K)]
    layout = GridLayout(ROWS, COLS, TW, TH, OW, OH)
    grids = [GridDecoderC(p, layout, [0]) for p in photos]
    album = decoder.Album([(p, ROWS, COLS, OW, OH) for p in photos])
    def in_turn():
        for g in grids:
            g.decode(); g.wait()
    def enqueued():
        for g in grids:
            g.decode()
        for g in grids:
            g.wait()
    def one_album():
        album.run(); album.status()
    forms = [("grids, in turn", in_turn), ("grids, enqueued", enqueued), ("album", one_album)]
    for _, f in forms:      # warm-up: code objects, pools
        f(); f()
    same = all(np.array_equal(a, b) for k in (0, K - 1) for a, b in zip(album.planes(k), grids[k].planes()))
    R = 10 if K < 16 else 6
    ms = {n: [] for n, _ in forms}
    paste = []
    for r in range(R):
        for n, f in forms:
            ms[n].append(clock(f))
        paste.append(album.paste_timing_us())
    say("")
    say("K = %d photos (%d tiles, %.0f Mpixel), R = %d; album canvases equal the grids' (photos 0 and K - 1): %s" % (K, K * ROWS * COLS, K * OW * OH / 1e6, R, same))
    for n, _ in forms:
        a = np.array(ms[n])
        say("  %-16s mean %8.2f ms  median %8.2f  min %8.2f  max %8.2f   %7.0f Mpixel/s of composed photos at the mean" % (n, a.mean(), np.median(a), a.min(), a.max(), K * OW * OH / a.mean() / 1e3))
    p = np.array(paste)
    moved = 2 * K * 1.5 * OW * OH      # read + write of every output sample
    say("  paste launch     mean %8.1f us  min %8.1f  max %8.1f   (%d jobs; %.0f MB read + written -> %.2f TB/s at the mean)" % (p.mean(), p.min(), p.max(), K * ROWS * COLS * 3, moved / 1e6, moved / p.mean() / 1e6))
    best = min(np.mean(ms["grids, in turn"]), np.mean(ms["grids, enqueued"]))
    say("  album / best grid form at the mean: %.3f" % (np.mean(ms["album"]) / best))
    for g in grids:
        g.free()
    album.free()
    b = decoder.Batch([t for p in photos for t in p])      # the album's launch set without the paste: where its time goes
    b.run(); b.status(); b.run(); b.status()
    t = b.kernel_timing_us()
    say("  the %d tiles as a plain Batch, device time per kernel (us): %s" % (K * ROWS * COLS, "  ".join("%s %.0f" % (k, v) for k, v in t.items())))
    b.free()
out.close()
