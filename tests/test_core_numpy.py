"""The inputs of tests/test_gpu_core_seams.py are not vacuous, shown without a GPU: at every size of the seam table
(tests/core_fixtures.py) the oracle and the plain numpy definitions (tests/core_numpy.py) agree, and the cases have the properties
the GPU tests rely on -- RANSAC cases with a real inlier set and a second hypothesis phase, ANMS cases with a radius tie at the
decision rank, with points nothing dominates and with negative responses, compaction masks whose odd bytes lie in a counted prefix,
colour points on every side of the clamp.  The counts that prove each property stand in the assertion messages."""
import functools

import numpy as np
import pytest

import core_fixtures as cf
import core_numpy as cn
from geom_fixtures import BASELINE, K4


# ------------------------------------------------------------------------------------------------------------------ the table
def test_seam_table_has_the_sizes_the_kernels_constants_give():
    assert cf.sizes("compact") == [0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049]
    assert cf.sizes("anms") == [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1025]
    assert cf.sizes("points") == [0, 1, 63, 64, 65, 255, 256, 257, 1025]
    assert cf.sizes("colors") == [1, 255, 256, 257]
    assert cf.sizes("fransac") == [17, 63, 64, 65, 66, 67, 255, 256, 257, 799]
    assert cf.sizes("pnp") == [5, 6, 7, 8, 63, 64, 65, 255, 256, 257]
    assert cf.sizes("ba") == [2, 63, 64, 65, 255, 256, 257, 511, 512, 513]
    assert set(cf.SOR_CASES) == {(n, k) for n in (255, 256, 257) for k in (8, n - 2, n - 1, n, 300)} | {(65, 64), (64, 63)}
    # the segment length changes where the table says it does
    assert [cf.compact_seg(n) for n in (1, 1024, 1025, 2048, 2049)] == [64, 64, 128, 128, 192]
    for seams in cf.SEAMS.values():
        assert all(s.n <= 2100 and s.probes and ".hip:" in s.source for s in seams)


# ------------------------------------------------------------------------------------------------------------------ compaction
@pytest.mark.parametrize("n", cf.sizes("compact"))
def test_compact_definition_equals_the_push_back_loop(n):
    """There is no oracle entry for compaction: the definition is held to the reference's own form, a loop that appends."""
    arrays = cf.compact_arrays(n)
    for kind in cf.MASK_KINDS:
        mask = cf.compact_mask(n, kind)
        assert mask.dtype == np.uint8 and len(mask) == n
        rows = [i for i in range(n) if mask[i] == 1]
        for got, a in zip(cn.compact(mask, *arrays), arrays):
            assert got.shape == (len(rows), a.shape[1]) and all(np.array_equal(g, a[i]) for g, i in zip(got, rows)), (n, kind)
    assert cf.compact_mask(n, "ones").sum() == n and not cf.compact_mask(n, "zeros").any()
    if n:
        assert np.flatnonzero(cf.compact_mask(n, "first")).tolist() == [0] and np.flatnonzero(cf.compact_mask(n, "last")).tolist() == [n - 1]


@pytest.mark.parametrize("n", [n for n in cf.sizes("compact") if n >= 65])
def test_odd_mask_bytes_lie_in_the_counted_prefix_of_a_later_segment(n):
    mask = cf.compact_mask(n, "odd")
    seg = cf.compact_seg(n)
    prefix_end = (n - 1) // seg * seg                      # everything before the LAST segment is some segment's prefix
    assert prefix_end >= 64
    odd = {v: int((mask[:prefix_end] == v).sum()) for v in cf.ODD_BYTES}
    assert all(c > 0 for c in odd.values()), (n, seg, odd)
    # and each odd value stands beside a 0x01 inside one dword; with a prefix of 960 bytes or more, in every byte lane of a dword
    lanes = {v: sorted({int(p) % 4 for p in np.flatnonzero(mask[:prefix_end] == v)}) for v in cf.ODD_BYTES if v}
    beside = all(mask[p - 1] == 1 for v in cf.ODD_BYTES if v for p in np.flatnonzero(mask[:prefix_end] == v) if p % 4)
    assert beside and all(len(l) >= (4 if prefix_end >= 960 else 2) for l in lanes.values()), (n, prefix_end, lanes)
    assert 0 < (mask == 1).sum() < n, (n, int((mask == 1).sum()))


# ------------------------------------------------------------------------------------------------------------------ ANMS
@functools.lru_cache(maxsize=None)
def _radii(kind, n):
    return cn.anms_radii(*cf.anms_input(kind, n))


@pytest.mark.parametrize("n", cf.sizes("anms"))
@pytest.mark.parametrize("kind", cf.ANMS_KINDS)
def test_anms_oracle_equals_restatement(orc, kind, n):
    xy, resp = cf.anms_input(kind, n)
    order, r2 = _radii(kind, n)
    for keep in cf.anms_keeps(n):
        got, _ = orc.anms(xy, resp, keep)
        ref = cn.anms_select(order, r2, keep)
        assert np.array_equal(got, ref), (kind, n, keep, len(got), len(ref))
        assert len(got) == n if n <= keep else len(got) >= min(keep + 1, n)


def test_anms_cases_have_ties_undominated_points_and_negative_responses():
    tie_cases = lone_cases = first_only_cases = negative_cases = total = 0
    for kind in cf.ANMS_KINDS:
        for n in cf.sizes("anms"):
            xy, resp = cf.anms_input(kind, n)
            order, r2 = _radii(kind, n)
            total += 1
            negative_cases += int((resp < 0).any() and (resp > 0).any())
            lone_cases += int(np.isinf(r2[1:]).any())                      # a point besides the first that nothing dominates
            thr = (resp[order] * np.float32(1.11)).astype(np.float32)
            n_dom = np.array([(resp[order[:s]] > thr[s]).sum() for s in range(n)])
            first_only_cases += int(((n_dom == 1) & (np.arange(n) > 0)).any())  # ... whose only dominator is the first sorted point
            tie_cases += sum(len(cn.anms_select(order, r2, keep)) > keep + 1 for keep in cf.anms_keeps(n) if keep < n - 1)
    counts = dict(total=total, tie=tie_cases, undominated=lone_cases, first_only=first_only_cases, negative=negative_cases)
    assert tie_cases >= 10 and lone_cases >= 10 and first_only_cases >= 5 and negative_cases >= 10, counts
    # a tie at the decision rank of the lattice in particular: more than keep + 1 come back
    order, r2 = _radii("lattice", 257)
    assert len(cn.anms_select(order, r2, 128)) > 129, len(cn.anms_select(order, r2, 128))


# ------------------------------------------------------------------------------------------------------------------ colours
@pytest.mark.parametrize("w,h,c", cf.COLOR_IMAGES)
def test_colors_oracle_equals_restatement(orc, w, h, c):
    img = cf.color_image(w, h, c)
    edge = cf.color_edge_points(w, h)
    assert np.abs(edge).max() < 2 ** 31 and not np.isnan(edge).any()
    outside = int(((edge[:, 0] < 0) | (edge[:, 0] >= w) | (edge[:, 1] < 0) | (edge[:, 1] >= h)).sum())
    toward_zero = int(((edge > -1) & (edge < 0)).any(axis=1).sum())         # truncation gives 0 here, floor would give -1
    assert outside >= 14 and toward_zero >= 3, (outside, toward_zero)
    for n in cf.sizes("colors") + [len(edge)]:
        xy = cf.color_points(w, h, n)
        assert len(xy) == n
        got, ref = orc.get_colors(img, xy), cn.get_colors(img, xy)
        assert np.array_equal(got, ref), (w, h, c, n, np.flatnonzero((got != ref).any(axis=1)))
    for p in edge:                                                          # n = 1 takes each edge point in turn on the GPU
        assert np.array_equal(orc.get_colors(img, p[None]), cn.get_colors(img, p[None])), p
    # the edge points read the pixels a clamp gives, and a wrong clamp would read different values
    ref = cn.get_colors(img, edge)
    assert np.array_equal(ref[0], ref[1]) and np.array_equal(ref[0, :c], img[int(h / 2 + 0.25), 0, :3].astype(np.float32)[:c])
    assert np.array_equal(ref[4, :c], img[int(h / 2 + 0.25), w - 1, :3].astype(np.float32)[:c])


# ------------------------------------------------------------------------------------------------------------------ transform
@pytest.mark.parametrize("n", cf.sizes("points"))
def test_transform_oracle_within_one_ulp_of_float64_numpy(orc, n):
    pts = cf.transform_input(n)
    got, ref = orc.transform_points(cf.RT, pts), cn.transform_points(cf.RT, pts)
    d = cf.ulp_distance(got, ref)
    assert got.shape == ref.shape == (n, 3)
    assert n == 0 or d.max() <= 1, f"n = {n}: {int((d > 0).sum())} of {d.size} components differ, the worst by {int(d.max())} ulp"


# ------------------------------------------------------------------------------------------------------------------ triangulation
@pytest.mark.parametrize("n", cf.sizes("points"))
def test_triangulate_oracle_within_the_standing_tolerance_of_the_svd(orc, n):
    P1, P2 = orc.stereo_projections(*K4, BASELINE)
    a, b, zero, neg = cf.tri_input(n)
    xyz, h = orc.triangulate(P1, P2, a, b)
    ref_xyz, ref_v = cn.triangulate(P1, P2, a, b)
    cf.check_dlt(xyz, h, ref_xyz, ref_v, zero, ("oracle", n))
    if n:
        assert len(zero) >= 1 and (n == 1 or len(neg) >= 1)
        assert (np.abs(ref_v[zero, 3]) < 1e-12).all(), ref_v[zero, 3]       # points at infinity ...
        assert (ref_xyz[neg, 2] < 0).all() and np.isfinite(ref_xyz[neg]).all()      # ... and points behind the camera
    if n >= 2 * cf.WAVE:                                                    # both kinds at both ends of a wave
        assert {int(i) % cf.WAVE for i in zero} >= {0, cf.WAVE - 1} and {int(i) % cf.WAVE for i in neg} >= {0, cf.WAVE - 1}


# ------------------------------------------------------------------------------------------------------------------ RANSAC
@functools.lru_cache(maxsize=None)
def _fransac(orc, n, thr):
    x1, x2, gt, seed = cf.fransac_case(n, thr)
    return orc.fransac(x1, x2, thr, seed=seed), gt


@functools.lru_cache(maxsize=None)
def _pnp(orc, n):
    X, x, gt, err, seed = cf.pnp_case(n)
    return orc.pnp_ransac(X, x, K4, reproj_err=err, seed=seed), gt


@pytest.mark.parametrize("thr", cf.FRANSAC_THRESHOLDS)
@pytest.mark.parametrize("n", cf.sizes("fransac"))
def test_fransac_case_has_a_real_answer(orc, n, thr):
    (cnt, mask, F, iters), gt = _fransac(orc, n, thr)
    assert 0 < cnt < n and cnt == int(mask.sum()), (n, thr, cnt)
    assert (mask.astype(bool) & gt).sum() >= 0.8 * gt.sum(), (n, thr, cnt, int(gt.sum()))
    assert np.abs(F).max() > 0 and 0 < iters <= 1000


@pytest.mark.parametrize("n", cf.sizes("pnp"))
def test_pnp_case_has_a_real_answer(orc, n):
    (cnt, rvec, tvec, inl, iters), gt = _pnp(orc, n)
    # a hypothesis needs more than four inliers, so five points are all or nothing; every larger case leaves its outliers out
    assert (cnt == 5 if n == 5 else 5 <= cnt < n) and len(inl) == cnt, (n, cnt)
    assert len(np.setdiff1d(inl, gt)) == 0 and np.all(np.diff(inl) > 0), (n, inl)
    assert 0 < iters <= 100 and np.abs(tvec).max() > 0


def test_some_ransac_cases_run_the_second_hypothesis_phase(orc):
    f_iters = {(n, thr): _fransac(orc, n, thr)[0][3] for n in cf.sizes("fransac") for thr in cf.FRANSAC_THRESHOLDS}
    p_iters = {n: _pnp(orc, n)[0][4] for n in cf.sizes("pnp")}
    assert (cf.F_PHASE_A, cf.PNP_PHASE_A) == (64, 32), "the existing tests quote these two"
    assert sum(v > cf.F_PHASE_A for v in f_iters.values()) >= 2 and min(f_iters.values()) <= cf.F_PHASE_A, f_iters
    assert sum(v > cf.PNP_PHASE_A for v in p_iters.values()) >= 1 and min(p_iters.values()) <= cf.PNP_PHASE_A, p_iters
