"""tests/project_ref.py - the NumPy restatement of the projective stage's integer arithmetic (include/heif_hipdec.h, hipdec_tensor_project) - against
PIL.Image.transform(size, Image.Transform.PERSPECTIVE | QUAD, data, resample, fillcolor) of Pillow itself, bit for bit: zero differing samples, no tolerance.

Sources 1 x 1, 1 x 7, 7 x 5, 33 x 17 and 64 x 48; outputs 1 x 1, 5 x 7 and 65 x 17; NEAREST, BILINEAR and BICUBIC.  PERSPECTIVE maps: the identity, an
affine-only map (a6 = a7 = 0), keystone in x, in y and in both, a map whose denominator runs from about 0.25 to 4 across the output, a map partly outside
and one wholly outside.  QUAD: the source's own corners, jittered corners, a non-convex quad and a quad outside - Pillow is given the CORNERS, the
restatement the coefficients of project_ref.quad_map, so the helper is pinned with the transform.

The pin holds on x86-64 builds of Pillow (see tests/test_warp_ref.py on fused multiply-adds elsewhere)."""
import numpy as np
import pytest

import project_ref as pr

Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: nothing to pin tests/project_ref.py to")

SOURCES = [(1, 1), (1, 7), (7, 5), (33, 17), (64, 48)]   # (width, height)
OUTPUTS = [(1, 1), (5, 7), (65, 17)]
FILTERS = [pr.NEAREST, pr.BILINEAR, pr.BICUBIC]
PIL_FILTER = {pr.NEAREST: Image.NEAREST, pr.BILINEAR: Image.BILINEAR, pr.BICUBIC: Image.BICUBIC}
FILL = (7, 201, 96)


def _source(size, seed):
    return np.random.default_rng(seed).integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)


def _pil(src, method, data, size, filt, fill=FILL):
    return np.asarray(Image.fromarray(src).transform(size, method, data=tuple(float(v) for v in data), resample=PIL_FILTER[filt], fillcolor=fill))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("src_size", SOURCES, ids=lambda s: "src%dx%d" % s)
def test_every_perspective_class_is_pillow_bit_for_bit(src_size, filt):
    src = _source(src_size, 11 * src_size[0] + src_size[1])
    for size in OUTPUTS:
        for name, m in pr.perspective_classes(src_size, size):
            assert not pr.refused(m, pr.PERSPECTIVE, size), (name, src_size, size)
            got, inside = pr.project(src, m, pr.PERSPECTIVE, size, filt, FILL)
            exp = _pil(src, Image.Transform.PERSPECTIVE, m, size, filt)
            assert int((got != exp).sum()) == 0, (name, src_size, size, filt, int((got != exp).sum()))
            if name == "all_outside":
                assert not inside.any() and (got == np.asarray(FILL, np.uint8)).all()
            if name == "identity" and size == src_size:
                assert inside.all() and np.array_equal(got, src)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("src_size", SOURCES, ids=lambda s: "src%dx%d" % s)
def test_every_quad_class_is_pillow_bit_for_bit_from_the_corners(src_size, filt):
    src = _source(src_size, 7 * src_size[0] + src_size[1])
    for size in OUTPUTS:
        for name, corners in pr.quad_classes(src_size, size):
            m = pr.quad_map(corners, size)
            assert not pr.refused(m, pr.QUAD, size), (name, src_size, size)
            got, inside = pr.project(src, m, pr.QUAD, size, filt, FILL)
            exp = _pil(src, Image.Transform.QUAD, corners, size, filt)
            assert int((got != exp).sum()) == 0, (name, src_size, size, filt, int((got != exp).sum()))
            if name == "outside":
                assert not inside.any()
            if name == "own_corners":
                assert inside.all()


def test_the_classes_are_what_their_names_say():
    """the comparison cannot pass on fill alone, the denominators span what is claimed, and `partly` is partly"""
    for src_size in SOURCES[2:]:
        size = (65, 17)
        src = np.zeros((src_size[1], src_size[0], 3), np.uint8)
        cls = dict(pr.perspective_classes(src_size, size))
        for name in ("identity", "affine_only", "keystone_x", "keystone_y", "keystone_both", "denominator_quarter_to_four", "partly_outside"):
            inside = pr.project(src, cls[name], pr.PERSPECTIVE, size, pr.BILINEAR)[1]
            assert inside.any(), (name, src_size)
        for name in ("keystone_x", "keystone_y", "keystone_both"):
            inside = pr.project(src, cls[name], pr.PERSPECTIVE, size, pr.BILINEAR)[1]
            assert 2 * int(inside.sum()) >= inside.size, (name, src_size)
        part = pr.project(src, cls["partly_outside"], pr.PERSPECTIVE, size, pr.BILINEAR)[1]
        assert part.any() and not part.all()
        a = cls["denominator_quarter_to_four"]
        d0, d1 = a[6] * 0.5 + 1.0, a[6] * (size[0] - 0.5) + 1.0
        assert 1.0 <= d0 < 1.05 and 4.6 < d1 <= 4.75      # numerators scaled by 0.25: the quotient's scale runs from about 0.25 ... to 1 / 4.7 of it
        assert cls["affine_only"][6:] == (0.0, 0.0) and cls["keystone_x"][7] == 0.0 and cls["keystone_y"][6] == 0.0
        q = dict(pr.quad_classes(src_size, size))
        for name in ("own_corners", "jittered", "non_convex"):
            inside = pr.project(src, pr.quad_map(q[name], size), pr.QUAD, size, pr.BICUBIC)[1]
            assert 4 * int(inside.sum()) >= inside.size, (name, src_size)


@pytest.mark.parametrize("filt", FILTERS)
def test_random_maps_are_pillow_bit_for_bit(filt):
    rng = np.random.default_rng(177)
    for k in range(24):
        src_size = (int(rng.integers(1, 40)), int(rng.integers(1, 40)))
        size = (int(rng.integers(1, 40)), int(rng.integers(1, 40)))
        src = _source(src_size, 100 + k)
        fill = tuple(int(v) for v in rng.integers(0, 256, 3))
        jit = lambda: rng.uniform(-0.3, 0.3)
        sw, sh = src_size
        corners = (jit() * sw, jit() * sh, jit() * sw, (1 + jit()) * sh, (1 + jit()) * sw, (1 + jit()) * sh, (1 + jit()) * sw, jit() * sh)
        m = pr.quad_map(corners, size)
        got, _ = pr.project(src, m, pr.QUAD, size, filt, fill)
        assert int((got != _pil(src, Image.Transform.QUAD, corners, size, filt, fill)).sum()) == 0, (k, "quad", corners, size)
        p = pr.keystone(src_size, size, rng.uniform(-0.6, 1.5), rng.uniform(-0.6, 1.5), rng.uniform(0.5, 1.5))
        if k % 3 == 0:
            p = p[:6] + (0.0, 0.0)
        p = (p[0], rng.uniform(-0.3, 0.3), p[2], rng.uniform(-0.3, 0.3)) + p[4:]
        assert not pr.refused(p, pr.PERSPECTIVE, size)
        got, _ = pr.project(src, p, pr.PERSPECTIVE, size, filt, fill)
        assert int((got != _pil(src, Image.Transform.PERSPECTIVE, p, size, filt, fill)).sum()) == 0, (k, "perspective", p, size)


def test_a_perspective_map_without_a6_a7_is_the_affine_restatement_for_the_double_filters():
    """division by exactly 1.0 is exact: BILINEAR and BICUBIC give tests/warp_ref.py's bytes for m = a[0 .. 5]"""
    import warp_ref as wr
    src = _source((33, 17), 4)
    for size in OUTPUTS:
        for name, m, _ in wr.map_classes((33, 17), size):
            for filt in (pr.BILINEAR, pr.BICUBIC):
                got, gin = pr.project(src, tuple(m) + (0.0, 0.0), pr.PERSPECTIVE, size, filt, FILL)
                exp, ein = wr.warp(src, m, size, filt, FILL)
                assert np.array_equal(got, exp) and np.array_equal(gin, ein), (name, size, filt)


def test_the_refusals_a_map_decides():
    ident = (1.0, 0, 0, 0, 1.0, 0, 0, 0)
    size = (16, 8)
    assert not pr.refused(ident, pr.PERSPECTIVE, size) and not pr.refused(ident, pr.QUAD, size)
    assert pr.refused(ident, 2, size) and pr.refused(ident, -1, size) and pr.refused(ident, pr.QUAD, size, reserved=1)
    for i in range(8):
        for bad in (float("nan"), float("inf"), -float("inf"), 32000.0, -40000.0):
            m = list(ident)
            m[i] = bad
            assert pr.refused(m, pr.PERSPECTIVE, size) and pr.refused(m, pr.QUAD, size), (i, bad)
    assert pr.refused((1, 0, 31985.0, 0, 1, 0, 0, 0), pr.PERSPECTIVE, size) and not pr.refused((1, 0, 31983.5, 0, 1, 0, 0, 0), pr.PERSPECTIVE, size)
    assert pr.refused((0, 0, 0, 0, 31993.0, 0, 1, 0), pr.QUAD, size) and not pr.refused((0, 0, 0, 0, 31991.0, 0, 1, 0), pr.QUAD, size)
    assert pr.refused((0, 0, 0, 250.0, 0, 0, 0, 1.0), pr.QUAD, size)                      # the xc * yc term: 250 * 16 * 8 = 32000 at the far corner only
    assert not pr.refused((0, 0, 0, 249.0, 0, 0, 0, 1.0), pr.QUAD, size)
    # the denominator: 1 - x / 16 is 0 at the right corners, 1 - x / 16.00001 is 6e-7 there (below 2^-20), 1 - x / 16.001 is 6e-5
    assert pr.refused((1, 0, 0, 0, 1, 0, -1.0 / 16, 0), pr.PERSPECTIVE, size)
    assert pr.refused((1, 0, 0, 0, 1, 0, -1.0 / 16.00001, 0), pr.PERSPECTIVE, size)
    assert pr.refused((1, 0, 0, 0, 1, 0, 0, -0.2), pr.PERSPECTIVE, size)                  # negative at the lower corners
    assert not pr.refused((0.001, 0, 0, 0, 0.001, 0, -1.0 / 16.001, 0), pr.PERSPECTIVE, size)
    assert pr.refused((1, 0, 0, 0, 1, 0, -1.0 / 16.001, 0), pr.PERSPECTIVE, size)          # ... but 16 / 6e-5 is far above 32000: the corner rule
    assert not pr.refused((1, 0, 0, 0, 1, 0, -1.0 / 16, 0), pr.QUAD, size)                 # QUAD has no denominator: a6 is a coefficient of yin


def test_the_exact_solution_satisfies_its_system():
    start = [(3.0, 5.0), (210.0, 11.0), (200.0, 190.0), (17.0, 222.0)]
    end = [(0.0, 0.0), (223.0, 0.0), (223.0, 223.0), (0.0, 223.0)]
    a = pr.perspective_map_exact(start, end)
    for (sx, sy), (ex, ey) in zip(start, end):
        xin, yin = pr.point([np.float64(v) for v in a], pr.PERSPECTIVE, np.float64(ex), np.float64(ey))
        assert abs(xin - sx) < 1e-9 and abs(yin - sy) < 1e-9
    np.testing.assert_allclose(pr.perspective_map(start, end), a, rtol=1e-10, atol=1e-13)
