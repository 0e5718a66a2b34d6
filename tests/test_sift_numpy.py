"""tests/sift_numpy.py, the restatement the SIFT kernels are held to, pinned against things that do not depend on it: Gaussian
blobs of known centre and width, an exact 90-degree rotation and a 2x nearest-neighbour enlargement of a rendered frame (angle
convention, descriptor rotation, octave packing, size formula), the parameter semantics, the accuracy of the svo_exp port, the
descriptor's range.  No GPU."""
import math

import numpy as np
import pytest

import sift_numpy as sn
from ros_stereo_slam_amd import synth


def blob(s, size=384, centre=(190.3, 187.6), amp=150.0, bg=40.0):
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    g = np.exp(-((x - centre[0]) ** 2 + (y - centre[1]) ** 2) / (2 * s * s))
    return np.rint(bg + amp * g).astype(np.uint8)


BLOB_S = [2.0, 2.8, 4.0, 5.7, 8.0, 11.3, 16.0]   # three octaves


def test_gaussian_blobs_give_one_keypoint_each_at_the_centre_with_monotone_size():
    sizes = []
    for s in BLOB_S:
        r = sn.sift(blob(s), descriptors=False)
        pts = np.unique(r["xy"], axis=0)
        assert len(pts) == 1, f"s = {s}: {len(pts)} key points"
        assert np.hypot(pts[0, 0] - 190.3, pts[0, 1] - 187.6) < 0.5, f"s = {s}: centre {pts[0]}"
        sizes.append(float(r["size"][0]))
    print("blob s -> size / s:", [round(z / s, 3) for z, s in zip(sizes, BLOB_S)])
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes


@pytest.fixture(scope="module")
def frame_result():
    img, _ = synth.Scene().render(np.eye(3), np.zeros(3), K=(360.0, 360.0, 320.0, 120.0), size=(640, 240))
    pyr = sn.build_pyramid(img)
    return img, pyr, sn.sift(img, pyramid=pyr)


def test_flat_image_gives_nothing():
    assert len(sn.sift(np.full((64, 96, 3), 77, np.uint8))["xy"]) == 0


def test_n_features_keeps_the_top_responses_with_ties(frame_result):
    img, pyr, full = frame_result
    resp = full["response"]
    order = np.sort(resp)[::-1]
    # a cut that falls inside a tie (two orientations of one extremum share a response)
    ties = np.flatnonzero(order[:-1] == order[1:])
    assert len(ties) > 0
    n = int(ties[len(ties) // 2]) + 1
    kept = sn.sift(img, n_features=n, pyramid=pyr, descriptors=False)
    assert len(kept["xy"]) > n
    keep = resp >= order[n - 1]
    assert len(kept["xy"]) == keep.sum()
    assert np.array_equal(kept["xy"], full["xy"][keep]) and np.array_equal(kept["response"], resp[keep])
    assert len(sn.sift(img, n_features=len(resp) + 5, pyramid=pyr, descriptors=False)["xy"]) == len(resp)


def test_output_order_is_octave_layer_row_column_bin(frame_result):
    _, _, r = frame_result
    assert len(r["xy"]) >= 500
    o = (r["octave"] & 255).astype(np.int64)
    o = np.where(o < 128, o, o - 256)
    layer = (r["octave"] >> 8) & 255
    scale = np.where(o >= 0, 1.0 / (1 << np.maximum(o, 0)), 2.0)
    row, col = np.floor(r["xy"][:, 1] * scale + 0.5), np.floor(r["xy"][:, 0] * scale + 0.5)
    key = np.stack([o, layer, row, col], axis=1)
    # the histogram bin of a peak: angle = 360 - 10 (bin + offset) with |offset| < 1/2 at a strict local maximum
    hbin = np.rint((360.0 - r["angle"].astype(np.float64)) / 10.0).astype(np.int64) % 36
    for a, b, ba, bb in zip(key[:-1], key[1:], hbin[:-1], hbin[1:]):
        assert tuple(a) <= tuple(b)
        if tuple(a) == tuple(b):
            assert ba < bb
    assert o.min() == -1 and layer.min() >= 1 and layer.max() <= 3


def test_svo_exp_port_is_within_one_ulp():
    x = np.linspace(-100.0, 0.0, 1_000_001)
    ref = np.array([math.exp(v) for v in x])
    err = np.abs(sn.svo_exp(x) - ref) / np.spacing(ref)
    assert err.max() <= 1.0
    assert sn.svo_exp(0.0) == 1.0 and sn.svo_exp(-800.0) == 0.0 and sn.svo_exp(800.0) == np.inf


def test_descriptor_range(frame_result):
    _, _, r = frame_result
    d = r["desc"]
    assert d.dtype == np.float32 and d.shape == (len(r["xy"]), 128)
    assert np.array_equal(d, np.rint(d)) and d.min() >= 0 and d.max() <= 255
    # the renormalised vector has norm 512 before rounding; rounding moves each of 128 entries by at most 1/2, saturation
    # at 255 can only lower the norm
    nrm = np.sqrt((d.astype(np.float64) ** 2).sum(1))
    slack = 0.5 * math.sqrt(128) + 1e-3
    assert (nrm <= 512 + slack).all()
    assert (nrm[d.max(1) < 255] >= 512 - slack).all()


# ---- rotation and enlargement of a rendered frame ----
# Geometry.  pt is the doubled frame's pixel index halved (S18) while that pixel's centre lies at d / 2 - 1/4 of the input
# (S2), so every key point sits 1/4 px right of and below the image point it marks.  np.rot90 sends the image point (x, y) to
# (y, W - 1 - x): pt moves to (y, W - 1/2 - x).  It turns directions counter-clockwise as displayed; KeyPoint::angle
# runs clockwise (360 - the y-up histogram angle, S17), so angles drop by 90.  np.repeat(2) sends the image point x to
# 2x + 1/2: pt moves to 2 pt + 1/4, size doubles, the octave rises by one.
# Shares.  The doubled frame is sampled symmetrically under the rotation, so at octave -1 every key point must map; the higher
# octaves keep the even samples (S4), which the rotation turns into the odd ones -- a half-sample shift that moves marginal
# extrema across the contrast / edge / 0.8-peak tests, and a nearest-neighbour enlargement is not a band-limited rescale: for
# those at most a quarter may go unmatched.  None whose response exceeds twice the contrast threshold (0.08) may.  The rendered
# texture alone is too faint for that clause to bite (its largest response is about 0.05), so high-contrast structures are pasted
# onto the crop: discs cut by a chord (one straight side: one dominant gradient direction; a full disc or an ellipse has
# several near-equal orientation peaks, and which of them clear 0.8 of the maximum is not stable).  For the rotation they are
# 2 ... 3 px across, so that they are found in octave -1, where the rotation is exact; for the enlargement 6 ... 12 px, because
# a nearest-neighbour enlargement of a 2 px structure is a different shape (2 x 2 blocks), not the same one twice as large.
UNMATCHED_SHARE = 0.25


def _octave(packed):
    o = (packed & 255).astype(np.int64)
    return np.where(o < 128, o, o - 256)


def _correspond(a, b, mapxy, dang, doct, dsize):
    """-> per key point of a: (a counterpart exists in b, the nearest descriptor of b lies at its own image point)"""
    oa, ob = _octave(a["octave"]), _octave(b["octave"])
    exp = mapxy(a["xy"].astype(np.float64))
    nn = ((a["desc"][:, None, :] - b["desc"][None, :, :]) ** 2).sum(2).argmin(1)
    found, own = np.zeros(len(exp), bool), np.zeros(len(exp), bool)
    for i in range(len(exp)):
        d = np.hypot(b["xy"][:, 0] - exp[i, 0], b["xy"][:, 1] - exp[i, 1])
        tol = 0.5 * 2.0 ** (oa[i] + doct)   # half a pixel of the octave
        da = np.abs((b["angle"] - (a["angle"][i] + dang) + 180) % 360 - 180)
        found[i] = ((d <= tol) & (ob == oa[i] + doct) & (da <= 10) &
                    (np.abs(np.log2(b["size"] / (a["size"][i] * dsize))) <= 1 / 6)).any()
        own[i] = d[nn[i]] <= tol
    return found, own, oa


SPOTS = [(40.3, 50.6, 1), (120.7, 45.2, -1), (190.4, 70.9, 1), (60.2, 150.3, 1), (150.6, 160.8, -1), (200.1, 200.4, 1), (100.5, 110.5, 1)]


def crop_with_spots(radii):
    """a 240 x 240 crop of a rendered frame with white (+1) / black (-1) chord-cut discs of the given radii pasted on"""
    R, t = synth.corridor_trajectory(4, step=0.5)[3]
    img, _ = synth.Scene().render(R, t, K=(360.0, 360.0, 320.0, 120.0), size=(640, 240))
    F = img[:, 300:540, 0].astype(np.float64)
    y, x = np.mgrid[0:240, 0:240].astype(np.float64)
    for (cx, cy, sign), r in zip(SPOTS, radii):
        th = 0.7 * cx   # the direction of the straight side
        u, v = (x - cx) * np.cos(th) + (y - cy) * np.sin(th), -(x - cx) * np.sin(th) + (y - cy) * np.cos(th)
        g = np.clip(r - np.hypot(u, v) + 0.5, 0, 1) * np.clip(u + 0.2 * r + 0.5, 0, 1)   # one-pixel ramps
        F = F * (1 - g) + (255.0 if sign > 0 else 0.0) * g
    F = np.clip(np.rint(F), 0, 255).astype(np.uint8)
    return F, sn.sift(F)


def test_rotation_by_90_degrees():
    F, a = crop_with_spots([2.0, 2.6, 2.2, 2.8, 2.0, 2.4, 3.0])
    W = F.shape[1]
    b = sn.sift(np.ascontiguousarray(np.rot90(F)))
    found, own, oa = _correspond(a, b, lambda p: np.c_[p[:, 1], W - 0.5 - p[:, 0]], -90.0, 0, 1.0)
    strong = a["response"] > 2 * 0.04
    print(f"rotation: {len(found)} key points, unmatched {(~found).sum()} ({(~found & (oa == -1)).sum()} at octave -1), nearest "
          f"descriptor elsewhere {(~own).sum()}, strong {strong.sum()} of which unmatched {(~found & strong).sum()}")
    assert (oa == -1).sum() >= 200 and found[oa == -1].all() and own[oa == -1].all()
    assert strong.sum() > 0 and found[strong].all() and own[strong].all()
    assert (~found).mean() <= UNMATCHED_SHARE and (~own).mean() <= UNMATCHED_SHARE


def test_enlargement_by_two():
    F, a = crop_with_spots([6.0, 9.0, 7.0, 10.0, 6.0, 8.0, 12.0])
    b = sn.sift(np.ascontiguousarray(np.repeat(np.repeat(F, 2, 0), 2, 1)))
    found, own, oa = _correspond(a, b, lambda p: 2 * p + 0.25, 0.0, 1, 2.0)
    strong = a["response"] > 2 * 0.04
    print(f"enlargement: {len(found)} key points, unmatched {(~found).sum()}, nearest descriptor elsewhere {(~own).sum()}, "
          f"strong {strong.sum()} of which unmatched {(~found & strong).sum()}")
    assert strong.sum() > 0 and found[strong].all() and own[strong].all()
    assert (~found).mean() <= UNMATCHED_SHARE and (~own).mean() <= UNMATCHED_SHARE
