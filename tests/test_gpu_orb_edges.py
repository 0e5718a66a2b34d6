"""svo_orb_extract_batch in cv::ORB's shape on the images of tests/orb_fixtures.py: the branches of cv_select_kernel and
cv_blur_corners_kernel that the corridor scene never reaches (both selection fallbacks, partial ties, no cut, levels smaller
than a tile, dense and tied corners at tile borders, budgets below the level count), one extractor re-used over flat and dense
images, and run-to-run determinism.  Every output is compared bit for bit with the C oracle AND with the numpy restatement
(tests/orb_numpy.py); that each image reaches the branch it is named for is proven in tests/test_orb_numpy.py from the
restatement's per-level record, which the tests here print.

Not covered: cap_out below the feature budget.  svo_orb_extract_batch always passes n_features as cap_out to
svo_orb_cv_launch, so the C ABI (and capi.py) cannot reach it without new plumbing."""
import numpy as np
import pytest

import orb_fixtures as fx
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu

NAMES = ("xy", "octave", "response", "dir", "desc")


def _gpu_params(prm):
    return dict(n_features=prm["n_features"], fast_threshold=prm["fast_t"], n_levels=prm["n_levels"], scale_factor=prm["scale_factor"])


def _same(got, ref, what):
    """got: the library's (xy, octave, response, dir, desc); ref: (xy, octave, response, dir, angle, desc)."""
    assert len(got[0]) == len(ref[0]), what
    for a, b, name in zip(got, (ref[0], ref[1], ref[2], ref[3], ref[5]), NAMES):
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, name)


def _oracle(orc, img, prm, pat=None):
    return orc.orb_extract_cv(img, prm["n_features"], prm["fast_t"], prm["n_levels"], prm["scale_factor"], pattern=pat)


def _record(levels):
    return [{k: v for k, v in L.items() if k not in ("score", "cand")} for L in levels]


@pytest.mark.parametrize("name", list(fx.cases()))
def test_fixture_matches_oracle_and_restatement(ctx, orc, name):
    img, prm, _, ref, levels = fx.reference(name)
    print(name, "level 0:", _record(levels)[:1])
    got = ctx.orb_extract_batch([img], **_gpu_params(prm))[0]
    assert len(got[0]) <= prm["n_features"]
    _same(got, _oracle(orc, img, prm), "oracle")
    _same(got, ref, "orb_numpy")       # every image, not only those of at most 200 x 200: the reference is shared and cheap


@pytest.mark.parametrize("name", ["motif_ramp", "noise3", "geom_131x97_x1.2"])
def test_fixture_with_a_pattern_up_to_15(ctx, orc, name):
    img, prm, pat, ref, _ = fx.reference(name, True)
    ctx.orb_set_pattern(pat)
    try:
        got = ctx.orb_extract_batch([img], **_gpu_params(prm))[0]
    finally:
        ctx.orb_set_pattern(None)
    _same(got, _oracle(orc, img, prm, pat), "oracle")
    _same(got, ref, "orb_numpy")
    assert not np.array_equal(got[4], fx.reference(name)[3][5])


def test_one_extractor_three_launches_flat_beside_dense(ctx, orc):
    prm = dict(n_features=300, fast_t=20, n_levels=3, scale_factor=1.2)
    noise = [fx.noise3(seed=s) for s in (0, 1, 2, 3)]
    motif, flat = fx.motif(), fx.flat()
    fresh = capi.Context(0)            # each image alone, on a context of its own
    try:
        alone = {id(im): fresh.orb_extract_batch([im], **_gpu_params(prm))[0] for im in noise + [motif]}
    finally:
        fresh.close()
    for im in noise + [motif]:
        assert len(alone[id(im)][0]) > 100
        _same(alone[id(im)], _oracle(orc, im, prm), "alone against the oracle")
    for batch in (noise, [noise[0], flat, motif, flat], [flat] * 4):
        got = ctx.orb_extract_batch(batch, **_gpu_params(prm))
        assert len(got) == 4
        for im, g in zip(batch, got):
            if im is flat:
                assert len(g[0]) == 0
            else:
                for a, b, name in zip(g, alone[id(im)], NAMES):
                    assert np.array_equal(a, b), name


@pytest.mark.parametrize("name", ["motif", "noise3"])
def test_five_runs_on_one_context_are_identical(ctx, name):
    """The candidate list arrives in tile-completion order; the selection must not depend on it."""
    img, prm, _, ref, _ = fx.reference(name)
    runs = [ctx.orb_extract_batch([img], **_gpu_params(prm))[0] for _ in range(5)]
    _same(runs[0], ref, "orb_numpy")
    for r in runs[1:]:
        for a, b, what in zip(r, runs[0], NAMES):
            assert np.array_equal(a, b), what
