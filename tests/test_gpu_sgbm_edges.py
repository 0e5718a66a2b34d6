"""svo_sgbm_compute where test_gpu_sgbm.py's smooth textures never take it: every pre-filter cap regime, the penalty
clamps and int16 wrap-around of C and Lr, saturated sums (d = -1), ties everywhere, speckle windows on both sides of a
component's exact size, full-width LDS rows and the capacity refusals.  Every comparison is exact equality with the
numpy restatement tests/sgbm_numpy.py; every case first asserts, from the restatement alone, that its input reaches
the branch it was written for."""
import ctypes as C
from collections import deque

import numpy as np
import pytest

import sgbm_fixtures as fx
import sgbm_numpy as sn
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu

_refs = {}


def _params(**kw):
    p = sn.Params(speckle_window_size=0)
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _want(key, left, right, **kw):
    """(result, stages) of the restatement, computed once per (input name, parameters)."""
    k = (key, tuple(sorted(kw.items())))
    if k not in _refs:
        stages = {}
        _refs[k] = (sn.sgbm(left, right, _params(**kw), stages), stages)
    return _refs[k]


def _same(got, want, what=""):
    assert got.dtype == np.int16 and got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        at = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}{len(bad)} pixels differ, first {at}: got {got[at]} want {want[at]}")


def _check(ctx, key, left, right, **kw):
    want, stages = _want(key, left, right, **kw)
    kw.setdefault("speckle_window_size", 0)
    _same(ctx.sgbm(left, right, **kw), want)
    return want, stages


def _saturated_share(stages):
    return float((stages["S"].min(axis=2) == sn.SHRT_MAX).mean())


INPUTS = {
    "mixed": lambda: fx.mixed(150, 24),
    "unrelated": lambda: fx.unrelated(150, 24),
    "constant": lambda: fx.constant(90, 10),
    "stripes": lambda: fx.stripes(90, 10),
    "half_stripes": lambda: fx.half_stripes(120, 10),
}


# ---- 1. the pre-filter cap: below the floor of 15, odd / even, the last cap that fits a uchar, the wrapped range ----
@pytest.mark.parametrize("cap", [0, 1, 15, 16, 63, 127, 128, 200, 300])
@pytest.mark.parametrize("name", ["mixed", "unrelated"])
def test_pre_filter_cap(ctx, name, cap):
    left, right = INPUTS[name]()
    by_cap = {c: _want(name, left, right, num_disparities=16, pre_filter_cap=c)[0] for c in (15, 127, 200)}
    assert not np.array_equal(by_cap[127], by_cap[200]) and not np.array_equal(by_cap[127], by_cap[15])   # the cap acts
    _check(ctx, name, left, right, num_disparities=16, pre_filter_cap=cap)


# ---- 2. penalties: the clamps of R14 and two's-complement int16 storage of C, Lr and minLr ---------------------------
@pytest.mark.parametrize("p1,p2", [(0, 1), (-5, -1), (1, 2), (8, 400), (200, 3000)])
def test_penalties(ctx, p1, p2):
    left, right = INPUTS["mixed"]()
    _check(ctx, "mixed", left, right, num_disparities=16, p1=p1, p2=p2)


@pytest.mark.parametrize("name", ["mixed", "unrelated"])
def test_penalty_that_wraps_int16(ctx, name):
    """P2 = 32000: C = P2 + block sum wraps, Lr leaves int16 on the way down.  The stored Lr' and minLr' wrap; the
    sweep's sum takes the int L (R7: ``Sp[d] = sat16(Sp[d] + L0 + L1 + L2 + L3)`` with int L0..L3)."""
    left, right = INPUTS[name]()
    kw = dict(num_disparities=16, p1=24, p2=32000)
    _, stages = _want(name, left, right, **kw)
    assert stages["C"].min() < 0 and stages["S"].min() == -32768
    # some int L lies below int16, so that a sum of wrapped L would differ
    lmin = min(int(sn.path_costs(stages["C"], _params(**kw), r).min()) for r in range(5))
    assert lmin < -32768, lmin
    _check(ctx, name, left, right, **kw)


# ---- 3. saturation: sat16 of both sums, minS >= SHRT_MAX -> d = -1, disp2 and drow with d = -1 ------------------------
def _saturating(D):
    return fx.unrelated(D + 104, 14, seed=0, run=3)


@pytest.mark.parametrize("D", [16, 96, 160])   # PER = 1, 2, 4
def test_saturated_sums(ctx, D):
    left, right = _saturating(D)
    kw = dict(num_disparities=D, block_size=11, pre_filter_cap=127)
    _, stages = _want(f"sat{D}", left, right, **kw)
    share = _saturated_share(stages)
    assert 0.05 <= share <= 0.95, share
    _check(ctx, f"sat{D}", left, right, **kw)


@pytest.mark.parametrize("extra", [dict(uniqueness_ratio=10), dict(disp12_max_diff=2)], ids=["unique10", "lr2"])
def test_saturated_sums_with_the_later_checks(ctx, extra):
    left, right = _saturating(16)
    kw = dict(num_disparities=16, block_size=11, pre_filter_cap=127, **extra)
    _, stages = _want("sat16", left, right, **kw)
    assert 0.05 <= _saturated_share(stages) <= 0.95
    _check(ctx, "sat16", left, right, **kw)


# ---- 4. ties: the first d of the smallest S, the rightmost left pixel for disp2, the uniqueness product ---------------
@pytest.mark.parametrize("D", [16, 32])
@pytest.mark.parametrize("ratio", [-1, 0, 10, 50, 100])
@pytest.mark.parametrize("minD", [0, 1, -8])
@pytest.mark.parametrize("name", ["constant", "stripes", "half_stripes"])
def test_ties_and_uniqueness(ctx, name, minD, ratio, D):
    left, right = INPUTS[name]()
    kw = dict(min_disparity=minD, num_disparities=D)
    by_ratio = {r: _want(name, left, right, uniqueness_ratio=r, **kw) for r in {-1, 0, 10, 50, ratio}}
    assert np.array_equal(by_ratio[-1][0], by_ratio[10][0])   # a negative ratio reads as 10
    if name == "half_stripes":   # the ratio drops some pixels and keeps others
        valid = [float((by_ratio[r][0] != (minD - 1) * sn.DISP_SCALE).mean()) for r in (0, 10, 50)]
        assert valid[0] > valid[1] + 0.02 and valid[1] > valid[2] + 0.02 and valid[2] > 0.02, valid
    else:   # every band pixel has more than one smallest S
        S = by_ratio[ratio][1]["S"]
        assert ((S == S.min(axis=2, keepdims=True)).sum(axis=2) > 1).all()
        if name == "stripes":   # and the ratio acts on them
            assert not np.array_equal(by_ratio[-1][0], by_ratio[0][0])
    _check(ctx, name, left, right, uniqueness_ratio=ratio, **kw)


# ---- 5. speckles: every range, windows on both sides of a component's exact size, labels shared by a batch ----------
SPECKLE_KW = dict(num_disparities=48)


def _noisy_pairs():
    pairs = [fx.textured(160, 32, shift=5, seed=s, noise=20) for s in (11, 12, 13)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _component_sizes(d, new_val, max_diff):
    """Sizes of filterSpeckles' components by a flood fill (written apart from the restatement's csgraph labelling)."""
    h, w = d.shape
    seen = d == new_val
    sizes = []
    for y0, x0 in zip(*np.nonzero(~seen)):
        if seen[y0, x0]:
            continue
        n, q = 0, deque([(y0, x0)])
        seen[y0, x0] = True
        while q:
            y, x = q.popleft()
            n += 1
            for yy, xx in ((y + 1, x), (y - 1, x), (y, x + 1), (y, x - 1)):
                if 0 <= yy < h and 0 <= xx < w and not seen[yy, xx] and abs(int(d[yy, xx]) - int(d[y, x])) <= max_diff:
                    seen[yy, xx] = True
                    q.append((yy, xx))
        sizes.append(n)
    return sorted(sizes)


def _speckle_case(L, R, srange, which):
    """(window, expected n x h x w): the restatement's filter on its own median images."""
    new_val = (sn.Params().min_disparity - 1) * sn.DISP_SCALE
    med = [_want(f"noisy{k}", L[k], R[k], **SPECKLE_KW)[1]["median"] for k in range(len(L))]
    sizes = [s for s in _component_sizes(med[0], new_val, sn.DISP_SCALE * srange) if s >= 2]
    s_star = sizes[len(sizes) // 2]   # an actual component of pair 0: s* and s* - 1 sit on the two sides of the <=
    window = {"one": 1, "s*": s_star, "s*-1": s_star - 1, "all": 100000}[which]
    want = np.stack([sn.filter_speckles(m, new_val, window, sn.DISP_SCALE * srange) for m in med]) if window > 0 else np.stack(med)
    if which == "s*":
        below = sn.filter_speckles(med[0], new_val, s_star - 1, sn.DISP_SCALE * srange) if s_star > 1 else med[0]
        assert int((want[0] != below).sum()) >= s_star   # the component goes at s* and stays at s* - 1
    return window, want


@pytest.mark.parametrize("which", ["one", "s*", "s*-1", "all"])
@pytest.mark.parametrize("srange", [0, 1, 5, 100])
def test_speckle_windows(ctx, srange, which):
    L, R = _noisy_pairs()
    window, want = _speckle_case(L, R, srange, which)
    kw = dict(speckle_window_size=window, speckle_range=srange, **SPECKLE_KW)
    assert np.array_equal(want[0], sn.sgbm(L[0], R[0], _params(**kw)))   # the shortcut is the restatement's own result
    _same(ctx.sgbm(L[0], R[0], **kw), want[0])
    got = ctx.sgbm(L[..., None], R[..., None], **kw)   # three pairs: their labels share one parent array
    for k in range(3):
        _same(got[k], want[k], f"pair {k}: ")


# ---- 6. widths and capacity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3], ids=["grey", "bgr"])
def test_widest_image(ctx, c):
    left, right = fx.textured(2048, 3, shift=4, seed=7, c=c)   # the LDS rows of the cost and WTA kernels are full
    _check(ctx, f"w2048c{c}", left, right, num_disparities=16)


@pytest.mark.parametrize("n,w,h,kw", [(1, 2049, 3, dict(num_disparities=16)),
                                      (16, 2048, 160, dict(num_disparities=256, min_disparity=0))],
                         ids=["w2049", "cells"])
def test_capacity_refusals(ctx, n, w, h, kw):
    if n > 1:
        assert n * h * (w - kw["num_disparities"]) * kw["num_disparities"] > 2 ** 30
    img = np.zeros((n, h, w), np.uint8)
    out = np.full((n, h, w), -12345, np.int16)
    prm = capi.sgbm_params(**kw)
    rc = ctx.lib.svo_sgbm_compute(ctx._h, C.byref(prm), capi._ptr(img), capi._ptr(img), w, h, 1, n, capi._ptr(out), capi.MEM_HOST)
    assert rc == capi.SVO_ERR_CAPACITY
    assert "svo_sgbm_compute" in ctx.lib.svo_last_error().decode()
    assert (out == -12345).all()
    with pytest.raises(capi.SvoError) as e:   # and through the binding
        ctx.sgbm(*([img[..., None]] * 2 if n > 1 else [img[0]] * 2), **kw)
    assert e.value.code == capi.SVO_ERR_CAPACITY and "svo_sgbm_compute" in str(e.value)


# ---- 7. device memory -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["saturated", "ties"])
def test_device_memory_matches_host(ctx, case):
    import torch

    if case == "saturated":
        pairs = [fx.unrelated(120, 14, seed=s, run=3) for s in (0, 1)]
        kw = dict(num_disparities=16, block_size=11, pre_filter_cap=127, speckle_window_size=0)
        _, stages = _want("sat16", *_saturating(16), num_disparities=16, block_size=11, pre_filter_cap=127)
        assert 0.05 <= _saturated_share(stages) <= 0.95   # pair 0 is that input
    else:
        pairs = [fx.stripes(90, 10), fx.constant(90, 10)]
        kw = dict(num_disparities=16, uniqueness_ratio=10, speckle_window_size=0)
    L, R = (np.stack([p[k] for p in pairs])[..., None] for k in range(2))
    host = ctx.sgbm(L, R, **kw)
    for k in range(2):
        _same(host[k], sn.sgbm(L[k], R[k], _params(**kw)), f"pair {k}: ")
    dev = ctx.sgbm(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), **kw)
    assert dev.is_cuda and dev.dtype == torch.int16
    _same(dev.cpu().numpy(), host)
