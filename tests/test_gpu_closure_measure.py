"""svo_closure_measure (getLCMeasurement, dump.cpp:331-348) against the oracle's stages chained by hand: LK newest -> matched,
compaction by status, F-matrix RANSAC, compaction by mask, PnP-RANSAC, then Rodrigues / transpose / -R tvec and the quaternion
formula include/svo.h states, in numpy.  Every stage is bit-exact against the oracle on its own, so the composition is too."""
import ctypes as C

import numpy as np
import pytest

from closure_fixtures import K4, SEED, SIZE, make_pair, quat_of
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu
SETTINGS = [(0.1, 0.999), (1.0, 0.99)]      # the reference's (dump.cpp:340), and the front-end's first attempt


@pytest.fixture(scope="module")
def pair(ctx):
    return make_pair(ctx)


def oracle_chain(orc, pair, reproj, conf, f_thr=1.0):
    nxt, st, _, _ = orc.lk_track(pair["newest"], pair["matched"], pair["xy"])
    keep = st == 1
    ref, trk, p3 = pair["xy"][keep], nxt[keep], pair["xyz"][keep]
    if f_thr > 0:
        _, mask, _, _ = orc.fransac(ref, trk, f_thr, 0.99, 1000, SEED + 1)
        trk, p3 = trk[mask == 1], p3[mask == 1]
    ninl, rvec, tvec, _, _ = orc.pnp_ransac(p3, trk, K4, 100, reproj, conf, SEED + 2)
    R, t = orc.compose_camera_pose(rvec, tvec)
    return np.r_[t, quat_of(R)], len(trk), ninl


@pytest.mark.parametrize("reproj,conf", SETTINGS)
def test_closure_measure_is_the_oracle_chain(ctx, orc, pair, reproj, conf):
    import torch

    assert 250 <= len(pair["xy"]) <= 400
    want, ntrk_o, ninl_o = oracle_chain(orc, pair, reproj, conf)
    rc, meas, ntrk, ninl = ctx.measure_closure(pair["newest"], pair["matched"], pair["xy"], pair["xyz"], K4,
                                               pnp_reproj_err=reproj, pnp_confidence=conf, seed=SEED)
    assert rc == capi.SVO_OK and (ntrk, ninl) == (ntrk_o, ninl_o)
    assert np.array_equal(meas, want), (meas, want)
    assert meas[6] >= 0 and abs(np.linalg.norm(meas[3:]) - 1) < 1e-15
    true = pair["true"]
    ang = np.rad2deg(2 * np.arcsin(min(1.0, np.linalg.norm(meas[3:6] * true[6] - true[3:6] * meas[6]
                                                           - np.cross(true[3:6], meas[3:6])))))
    print(f"\n{reproj} px / {conf}: {ntrk} tracked, {ninl} inliers; against the generator's relative pose: translation "
          f"{np.linalg.norm(meas[:3] - true[:3]) * 1e3:.2f} mm, rotation {ang:.4f} deg")
    # the same from device memory
    dev = [torch.from_numpy(pair[k]).cuda() for k in ("newest", "matched", "xy", "xyz")]
    w, h = SIZE
    rc2, meas2, ntrk2, ninl2 = ctx.measure_closure(*dev, K4, size=(w, h, 1, len(pair["xy"])), pnp_reproj_err=reproj,
                                                   pnp_confidence=conf, seed=SEED)
    assert rc2 == capi.SVO_OK and (ntrk2, ninl2) == (ntrk, ninl) and np.array_equal(meas2, meas)
    # without the F-matrix filter (f_thr <= 0): the status-filtered set goes to PnP
    want0, ntrk0, ninl0 = oracle_chain(orc, pair, reproj, conf, f_thr=0.0)
    rc3, meas3, ntrk3, ninl3 = ctx.measure_closure(pair["newest"], pair["matched"], pair["xy"], pair["xyz"], K4, f_thr=0.0,
                                                   pnp_reproj_err=reproj, pnp_confidence=conf, seed=SEED)
    assert rc3 == capi.SVO_OK and (ntrk3, ninl3) == (ntrk0, ninl0) and np.array_equal(meas3, want0)


def test_too_few_inliers_is_tracking_lost(ctx, pair):
    prm = capi.closure_params(pnp_reproj_err=1e-6, seed=SEED)
    meas = np.full(7, -7.0)
    ntrk, ninl = C.c_int(-1), C.c_int(-1)
    w, h = SIZE
    keep = [np.ascontiguousarray(pair[k]) for k in ("newest", "matched", "xy", "xyz")]
    K = np.array(K4)
    rc = ctx.lib.svo_closure_measure(ctx._h, capi._ptr(keep[0]), capi._ptr(keep[1]), w, h, 1, capi._ptr(keep[2]),
                                     capi._ptr(keep[3]), len(keep[2]), capi._ptr(K), C.byref(prm), capi._ptr(meas),
                                     C.byref(ntrk), C.byref(ninl), capi.MEM_HOST)
    assert rc == capi.SVO_ERR_TRACKING_LOST
    assert np.array_equal(meas, np.full(7, -7.0))
    assert 0 <= ninl.value < 6 and ntrk.value > 100
    rc, m, _, _ = ctx.measure_closure(pair["newest"], pair["matched"], pair["xy"], pair["xyz"], K4, pnp_reproj_err=1e-6, seed=SEED)
    assert rc == capi.SVO_ERR_TRACKING_LOST and m is None
