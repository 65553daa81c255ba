"""libheif_amd/csrc/photo_lut.h - what the photometric stage derives from a value, an operation or a histogram alone, the very functions k_photo_apply
compiles for the device - as a stand-alone host program (tests/emu/photo_lut_asan.cc, its own main) built with g++ -fsanitize=address,undefined, in the
manner of tools/warp_tables_sanitizer.sh, against tests/photo_ref.py (which tests/test_photo_ref.py pins to Pillow).  Exhaustive where the space is small:
  the autocontrast table for all 32 640 pairs lo < hi;
  the contrast mean for sums that land on k + 0.5 exactly;
  the equalize table for histograms with w * h - H[last] at 254, 255, 256 and 509 .. 511;
  BLEND for every (D, V) at factors inside [0, 1], above, below and at the refusal bound; the point operations; the refusals.
A sanitizer report ends the program with a non-zero status, which fails the test.  CPU only."""
import functools
import os
import subprocess

import numpy as np

import photo_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _program():
    out_dir = os.path.join(ROOT, "build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "photo_lut_asan")
    tmp = "%s.%d.tmp" % (out, os.getpid())
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(ROOT, "libheif_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "photo_lut_asan.cc"), "-o", tmp])
    os.replace(tmp, out)
    return out


def _run(mode, text=""):
    r = subprocess.run([_program()] + ([mode] if mode else []), input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    assert not r.stderr, r.stderr.decode()[-2000:]
    return r.stdout


def test_the_self_check_runs_clean_under_the_sanitizers():
    assert b"PHOTO LUT SANITIZER OK" in _run(None)


def test_the_autocontrast_table_for_every_pair():
    got = np.frombuffer(_run("autocontrast"), np.uint8).reshape(-1, 256)
    pairs = [(lo, hi) for lo in range(256) for hi in range(lo + 1, 256)]
    assert len(pairs) == 32640 and got.shape[0] == 32640
    exp = np.stack([pr.autocontrast_lut(lo, hi) for lo, hi in pairs])
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [pairs[i] for i in bad[:8]]


def test_the_contrast_mean_where_it_lands_on_one_half():
    cases = [(2 * k + 1, 2) for k in range(255)]                                   # k + 0.5 from two pixels
    cases += [((2 * k + 1) * p // 2, p) for k in (0, 10, 127, 254) for p in (4, 64, 1 << 20, 224 * 224, 32766 * 32767)]   # ... and from many
    cases += [(s, 7) for s in range(0, 7 * 255 + 1, 3)] + [(255 * 32767 * 32767, 32767 * 32767), (0, 1), (255, 1)]
    got = np.frombuffer(_run("mean", "".join("%d %d\n" % c for c in cases)), np.uint8)
    assert got.tolist() == [pr.contrast_mean(s, p) for s, p in cases]
    assert got[:255].tolist() == list(range(1, 256))                               # half rounds up


def test_the_equalize_table_at_the_step_thresholds():
    rng = np.random.default_rng(3)
    hists = []
    for rest in (254, 255, 256, 509, 510, 511, 1, 0, 100000):
        for last in (255, 200, 3):
            for last_count in (1, 2, 1000):
                H = np.zeros(256, np.int64)
                if rest:
                    H[:last] = rng.multinomial(rest, np.ones(last) / last)
                H[last] = last_count
                hists.append(H)
    hists.append(np.bincount(rng.integers(0, 256, 33 * 17), minlength=256))
    single = np.zeros(256, np.int64)
    single[77] = 12
    hists.append(single)
    got = np.frombuffer(_run("equalize", "".join(" ".join(str(int(v)) for v in H) + "\n" for H in hists)), np.uint8).reshape(-1, 256)
    assert got.shape[0] == len(hists)
    for k, H in enumerate(hists):
        assert np.array_equal(got[k], pr.equalize_lut(H)), (k, H.tolist())
    ident = np.arange(256, dtype=np.uint8)
    assert np.array_equal(pr.equalize_lut(hists[0]), ident) and not np.array_equal(pr.equalize_lut(hists[9]), ident)   # 254: step 0; 255: step 1


def test_blend_for_every_pair_of_values():
    factors = [0.0, 1.0, 0.3, 0.5, 0.999, 1.0000001, 1.3, 1.9, 7.25, -0.5, -3.0, 1e-30, 65536.0, -65536.0, 0.1 + 0.2]
    got = np.frombuffer(_run("blend", "".join("%r\n" % f for f in factors)), np.uint8).reshape(len(factors), 256, 256)
    D, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for k, f in enumerate(factors):
        assert np.array_equal(got[k], pr.blend(D, V, f)), f


def test_the_point_operations_and_the_refusals():
    ops = [(pr.BRIGHTNESS, 0.4), (pr.BRIGHTNESS, 1.7), (pr.BRIGHTNESS, -2.0), (pr.INVERT, 0.0), (0, 0.0)]
    ops += [(pr.POSTERIZE, float(b)) for b in range(9)] + [(pr.SOLARIZE, t) for t in (0.0, 1.0, 100.5, 128.0, 255.0, 256.0, -4.0, 65536.0)]
    got = np.frombuffer(_run("point", "".join("%d %r\n" % o for o in ops)), np.uint8).reshape(len(ops), 256)
    sample = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    for k, (op, v) in enumerate(ops):
        exp = sample[0, :, 0] if op == 0 else pr.apply_op(sample, op, v)[0, :, 0]
        assert np.array_equal(got[k], exp), (op, v)
    checks = [(op, r, v) for op in range(-1, 12) for r in (0, 1) for v in (0.0, 1.0, 2.5, 8.0, 9.0, -1.0, 65536.0, 65536.5, -65536.5)]
    got = np.frombuffer(_run("check", "".join("%d %d %r\n" % c for c in checks)), np.uint8)
    for k, (op, r, v) in enumerate(checks):
        assert bool(got[k]) == (pr.refused(op, v) or (r != 0 and 1 <= op <= 9)), (op, r, v, got[k])
