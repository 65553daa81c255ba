"""libheif_amd/csrc/augment_lut.h - what the augment stage derives from a pixel, an operation or a radius alone, the very functions k_augment_hue and
k_augment_blur compile for the device - against tests/augment_ref.py (which tests/test_augment_ref.py pins to Pillow), two ways:
  the stand-alone host program tests/emu/augment_lut_asan.cc (its own main), built with g++ -fsanitize=address,undefined in the manner of
  tests/test_photo_lut_host.py: both HSV functions and the hue shift over a lattice of 52^3 pixels that holds both ends of every component, the box
  parameters over a radius sweep to the cap, single box passes over lines shorter and longer than the window at byte and row strides, the refusals;
  hipdec_gaussian_box of the built library (host only: no device is touched) over the same sweep.
A sanitizer report ends the program with a non-zero status, which fails the test.  CPU only."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import augment_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 5
SWEEP = [k / 200.0 for k in range(0, 1601)] + [0.1 + 0.2, 1.41, 1.42, 2.44, 2.45, 7.999999]


@functools.lru_cache(maxsize=None)
def _program():
    out_dir = os.path.join(ROOT, "build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "augment_lut_asan")
    tmp = "%s.%d.tmp" % (out, os.getpid())
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I" + os.path.join(ROOT, "libheif_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "augment_lut_asan.cc"), "-o", tmp])
    os.replace(tmp, out)
    return out


def _run(mode, text="", *args):
    r = subprocess.run([_program()] + ([mode] if mode else []) + [str(a) for a in args], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    assert not r.stderr, r.stderr.decode()[-2000:]
    return r.stdout


def _lattice(step=STEP):
    v = np.array(list(range(0, 255, step)) + [255], np.uint8)
    a, b, c = np.meshgrid(v, v, v, indexing="ij")
    return np.stack([a, b, c], axis=-1).reshape(1, -1, 3)


def test_the_self_check_runs_clean_under_the_sanitizers():
    assert b"AUGMENT LUT SANITIZER OK" in _run(None)


def test_both_hsv_functions_over_the_lattice():
    T = _lattice()
    got = np.frombuffer(_run("rgb2hsv", "", STEP), np.uint8).reshape(T.shape)
    assert int((got != ar.rgb2hsv(T)).sum()) == 0
    got = np.frombuffer(_run("hsv2rgb", "", STEP), np.uint8).reshape(T.shape)
    assert int((got != ar.hsv2rgb(T)).sum()) == 0


def test_the_hue_shift_over_the_lattice():
    shifts = [0, 1, 43, 85, 128, 213, 255]
    T = _lattice(7)
    got = np.frombuffer(_run("hue", "".join("%d 7\n" % d for d in shifts)), np.uint8).reshape((len(shifts),) + T.shape)
    for k, d in enumerate(shifts):
        assert int((got[k] != ar.hue(T, d)).sum()) == 0, d


def test_the_box_parameters_over_a_radius_sweep():
    got = np.frombuffer(_run("box", "".join("%r\n" % x for x in SWEEP)), np.uint32).reshape(-1, 3)
    assert got.shape[0] == len(SWEEP)
    bad = [(x, tuple(int(v) for v in got[k]), ar.gaussian_box(x)) for k, x in enumerate(SWEEP) if tuple(int(v) for v in got[k]) != ar.gaussian_box(x)]
    assert not bad, bad[:8]
    assert sorted(set(int(r) for r in got[:, 0])) == list(range(8))


def test_hipdec_gaussian_box_is_the_same_function():
    from libheif_amd import decoder
    for x in SWEEP:
        assert decoder.gaussian_box(x) == ar.gaussian_box(x), x
    lib = decoder._bind(decoder.load_library())
    r, ww, fw = C.c_int(), C.c_uint32(), C.c_uint32()
    for x in (float("nan"), float("inf"), -1e-9, 8.0000001):
        assert lib.hipdec_gaussian_box(x, C.byref(r), C.byref(ww), C.byref(fw)) == -1
    assert lib.hipdec_gaussian_box(1.0, None, C.byref(ww), C.byref(fw)) == -1


def test_single_box_passes_over_lines():
    rng = np.random.default_rng(8)
    cases = []
    for radius in (0, 0.1, 0.5, 1.0, 1.42, 2.0, 3.3, 5.0, 8.0):
        for n in (1, 2, 3, 7, 16, 33, 112):
            for stride in (1, 3, 340):
                cases.append((radius, n, stride, rng.integers(0, 256, n)))
    step = np.zeros(16, np.int64)
    step[8:] = 255
    cases.append((2.0, 16, 3, step))
    text = "".join("%r %d %d %s\n" % (c[0], c[1], c[2], " ".join(str(int(v)) for v in c[3])) for c in cases)
    got = np.frombuffer(_run("line", text), np.uint8)
    at = 0
    for radius, n, stride, vals in cases:
        r, ww, fw = ar.gaussian_box(radius)
        exp = ar.box_pass(vals, 0, r, ww, fw)
        assert np.array_equal(got[at:at + n], exp), (radius, n, stride)
        at += n
    assert at == got.size


def test_the_refusals():
    checks = [(op, r, v) for op in range(-1, 20) for r in (0, 1) for v in (0.0, 1.0, 2.5, 8.0, 8.5, 9.0, -1.0, 255.0, 256.0, 65536.0, 65536.5)]
    got = np.frombuffer(_run("check", "".join("%d %d %r\n" % c for c in checks)), np.uint8)
    for k, (op, r, v) in enumerate(checks):
        assert bool(got[k]) == (ar.refused(op, v) or (r != 0 and (1 <= op <= 9 or op in (ar.HUE, ar.GAUSSIAN_BLUR)))), (op, r, v, got[k])
