"""CPU check of the LDS-resident unit maps of the throughput parser (HIPDEC_PARSE_LDS_MAPS, implied by HIPDEC_PARSE_LDS_CTX): small stills whose
right / bottom CTBs lie partly outside the picture, minimum CB 8 with NxN 4x4 transform blocks (the single-unit fills), cu_qp_delta on, WPP on and
off, a dependent slice segment - parsed by the host emulation of that build under the work pool with HIPDEC_POOL_YIELD 1 (maps zeroed for every CTB,
the product default) and 0 (maps carried over the CTBs of one activation).  The five maps, the coefficients and the SAO parameters are compared
with the oracle, and so are the planes that the emulated pixel kernels make of the parse.  The oracle has no hand-off record and no units outside
the picture: the published maps in CTB / z-scan order INCLUDING those units, and the hand-off records, are compared byte for byte with the
register-file build's (libparse_emu.so) instead, and the units outside the picture are zero with the product default.  The raw maps and records
are read out of the emulated batch by tests/emu/unit_maps_probe.cc, a small library of its own built here on demand with the flags of
tests/emu/Makefile."""
import ctypes as C
import fcntl
import os
import subprocess
import numpy as np
import pytest

import test_parse_emu as T
import test_pipeline_emu as PE
from oracle import pyoracle as orc

# (width, height, encoder settings): ENC_DEFAULTS already has log2_min_cb 3, log2_min_tb 2 (NxN 4x4), cu_qp_delta 1, wpp 1
CASES = [(72, 40, dict(stress=1)), (200, 136, dict(stress=1)), (200, 136, dict(wpp=0)), (48, 48, dict(log2_ctb=4, log2_max_tb=4, stress=1)),
         (48, 48, dict(log2_ctb=5, stress=1, wpp=0)), (64, 64, dict(stress=1)), (200, 136, dict(dependent_segments=3, stress=1)),
         (72, 40, dict(cu_qp_delta=0, qp=12))]
IDS = ["%dx%d,%s" % (w, h, ",".join("%s=%s" % kv for kv in c.items())) for w, h, c in CASES]
_streams = {}
_libs = {}


def stream(k):
    if k not in _streams:
        w, h, cfg = CASES[k]
        _streams[k] = orc.encode(orc.synth_image(w, h, 8, 1, seed=700 + k), **cfg)
    return _streams[k]


def _probe():
    """libunit_maps_probe.so beside the emulation libraries, compiled with the flags of tests/emu/Makefile (same layout of the batch object)"""
    if "probe" in _libs: return _libs["probe"]
    emu = os.path.join(T.HERE, "emu")
    root = os.path.dirname(T.HERE)
    src, out = os.path.join(emu, "unit_maps_probe.cc"), os.path.join(emu, "libunit_maps_probe.so")
    with open(os.path.join(emu, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in (src, os.path.join(emu, "emu_batch.h"))):
            tmp = "%s.tmp.%d" % (out, os.getpid())
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-DHIPDEC_HOST_EMU=1",
                                   "-DHIPDEC_PARSE_INTER=1", "-I" + os.path.join(emu, "shim"), "-I" + emu, "-I" + os.path.join(root, "include"),
                                   "-I" + os.path.join(root, "libheif_amd", "csrc"), "-shared", "-o", tmp, src])
            os.replace(tmp, out)
    P = C.CDLL(out)
    P.emu_raw_unit_maps.restype = C.c_long
    P.emu_raw_unit_maps.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_long]
    _libs["probe"] = P
    return P


def _load(name):
    if name in _libs: return _libs[name]
    T.build_emu(name)
    L = C.CDLL(os.path.join(T.HERE, "emu", name))
    L.emu_create.restype = C.c_void_p
    L.emu_create.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
    L.emu_free.argtypes = [C.c_void_p]
    L.emu_run_parse.argtypes = [C.c_void_p]
    L.emu_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.emu_maps.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    L.emu_coeffs.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
    L.emu_sao.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
    _libs[name] = L
    return L


def raw_maps(L, s):
    """(info, the five published maps [ctbs, units per CTB] in z-scan order, hand-off records [ctbs, 16]) of one still"""
    arr = (C.c_char_p * 1)(s); sizes = (C.c_size_t * 1)(len(s)); err = C.create_string_buffer(512)
    h = L.emu_create(1, arr, sizes, err, 512)
    assert h, err.value.decode()
    try:
        assert L.emu_run_parse(h) == 0
        info = (C.c_int * 7)()
        L.emu_info(h, 0, info)
        w, hgt, ctb_w, ctb_h, log2_ctb, cf, nsub = list(info)
        units = 1 << (2 * (log2_ctb - 2))
        maps = [np.full(ctb_w * ctb_h * units, 0xee, np.uint8) for _ in range(5)]
        rec = np.zeros((ctb_w * ctb_h, 16), np.uint32)
        assert _probe().emu_raw_unit_maps(h, 0, *[m.ctypes.data for m in maps], rec.ctypes.data, maps[0].size) == maps[0].size
    finally:
        L.emu_free(h)
    return (w, hgt, ctb_w, ctb_h, log2_ctb), [m.reshape(ctb_w * ctb_h, units) for m in maps], rec


def inside_mask(w, hgt, ctb_w, ctb_h, log2_ctb):
    """[ctbs, units per CTB] in z-scan order: the unit's top-left sample lies inside the picture"""
    n = 1 << (log2_ctb - 2)
    m = np.zeros((ctb_w * ctb_h, n * n), bool)
    for c in range(ctb_w * ctb_h):
        for uy in range(n):
            for ux in range(n):
                z = sum(((ux >> b) & 1) << (2 * b) | ((uy >> b) & 1) << (2 * b + 1) for b in range(4))
                m[c, z] = ((c % ctb_w) * n + ux) * 4 < w and ((c // ctb_w) * n + uy) * 4 < hgt
    return m


@pytest.mark.parametrize("yield_ctbs", [1, 0])
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_lds_unit_maps_match_oracle_and_register_build(k, yield_ctbs, monkeypatch):
    monkeypatch.setenv("HIPDEC_PARSE_POOL", "1")
    monkeypatch.setenv("HIPDEC_POOL_YIELD", str(yield_ctbs))
    lds, rf = _load("libparse_emu_lds.so"), _load("libparse_emu.so")
    s = stream(k)
    monkeypatch.setattr(T, "_LIB", lds)
    status, got = T.run_emu([s])
    assert status == 0, "device status 0x%x" % status
    T.check_against_oracle(s, got[0])
    PE._check(s, PE.decode_emu([s])[0])   # planes (parse + pixel kernels of the same library: T._LIB) against the oracle
    info, maps, rec = raw_maps(lds, s)
    info_rf, maps_rf, rec_rf = raw_maps(rf, s)
    assert info == info_rf
    for name, a, b in zip(("size", "flags", "ipm", "ipmc", "qp"), maps, maps_rf):
        np.testing.assert_array_equal(a, b, err_msg="published map %s, LDS build against register build" % name)
    np.testing.assert_array_equal(rec, rec_rf, err_msg="hand-off records")
    if yield_ctbs == 1:
        outside = ~inside_mask(*info)
        if CASES[k][0] % (1 << info[4]) or CASES[k][1] % (1 << info[4]): assert outside.any()
        for name, a in zip(("size", "flags", "ipm", "ipmc", "qp"), maps):
            assert not a[outside].any(), "map %s: units outside the picture must be published as zero" % name
            if name == "size": assert a[~outside].all()   # every unit inside carries a CB size
