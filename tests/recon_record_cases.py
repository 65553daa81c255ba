"""The stills of the reconstruction-record tests (tests/test_recon_record_emu.py on the host emulation, tests/test_recon_record_gpu.py on the GPU)."""
from oracle import pyoracle as orc

# (width, height, chroma_format_idc, encoder settings): no size is a CTB multiple, so the picture edge clips the availability runs on both axes; `stress`
# mixes all transform sizes 4 .. 32, NxN luma quads and all intra modes
STILLS = [(w, h, cf, dict(stress=1, qp=qp)) for (w, h) in ((72, 40), (136, 72), (200, 136)) for cf in (1, 0) for qp in (22, 37)]
STILLS += [(136, 72, 1, dict(log2_ctb=4, log2_max_tb=4, num_slices=2, wpp=0, stress=1, qp=22)),    # a slice that starts inside a CTB row: above-right alone
           (136, 72, 1, dict(pcm_pct=30, qp=37))]                                                    # PCM units
IDS = ["%dx%d,cf%d,%s" % (w, h, cf, ",".join("%s=%s" % kv for kv in kw.items())) for w, h, cf, kw in STILLS]


def stream(k):
    w, h, cf, kw = STILLS[k]
    return orc.encode(orc.synth_image(w, h, 8, cf, seed=700 + k), **kw)
