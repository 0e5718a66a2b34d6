"""The numpy restatement of the duplicate filter and the replenishing step (tests/replenish_numpy.py) against brute force over all
pairs, and the proof that every fixture of tests/replenish_fixtures.py reaches the branch it is named for.  CPU only;
tests/test_gpu_replenish.py holds the kernels against the same restatement."""
import numpy as np
import pytest

import replenish_fixtures as rf
import replenish_numpy as rn

BOX, DISC = rn.BOX, rn.DISC


def brute(ref, new, radius, mode):
    """All pairs at once, from the definitions of svo.h (no artefact, no list)."""
    ref, new = np.asarray(ref, np.float32).reshape(-1, 2), np.asarray(new, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        if mode == BOX:
            r, q = ref.astype(np.float64)[None, :, :], new.astype(np.float64)[:, None, :]
            hit = (r[..., 0] > q[..., 0] - radius) & (r[..., 0] < q[..., 0] + radius) & (r[..., 1] > q[..., 1] - radius) & \
                  (r[..., 1] < q[..., 1] + radius)
        else:
            d = (ref[None, :, :] - new[:, None, :]).astype(np.float64)
            hit = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) < radius
    return hit.any(axis=1)


@pytest.mark.parametrize("mode", [BOX, DISC])
def test_restatement_equals_brute_force_on_random_sets(mode):
    seen = set()
    for seed, (n_ref, n_new) in enumerate([(0, 9), (1, 1), (40, 70), (300, 257), (65, 0), (1025, 64)]):
        c = rf.random_case(n_ref, n_new, mode, seed)
        keep = rn.dedup(c["ref"], c["new"], c["radius"], mode)
        assert keep.dtype == np.uint8 and keep.shape == (n_new,)
        assert np.array_equal(keep == 0, brute(c["ref"], c["new"], c["radius"], mode))      # no new x is 0 in these sets
        seen |= set(keep.tolist())
    assert seen == {0, 1}


def test_box_and_disc_part_on_the_corner():
    b, d = rf.box_corner(BOX), rf.box_corner(DISC)
    assert rn.dedup_box(b["ref"], b["new"], 5.0).tolist() == [0, 0, 0]
    assert rn.dedup_disc(d["ref"], d["new"], 5.0).tolist() == [1, 0, 1]


def test_box_boundary_is_strict():
    c = rf.box_edge()
    assert rn.dedup_box(c["ref"], c["new"], c["radius"]).tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1]


def test_disc_boundary():
    c = rf.disc_6_8()
    assert rn.dedup_disc(c["ref"], c["new"], c["radius"]).tolist() == [1, 0, 1, 1, 0, 1]
    exact, below, above = rf.disc_sqrt_ulp()
    assert rn.dedup_disc(exact["ref"], exact["new"], exact["radius"]).tolist() == [1, 1, 1]
    assert rn.dedup_disc(below["ref"], below["new"], below["radius"]).tolist() == [1, 1, 1]
    assert rn.dedup_disc(above["ref"], above["new"], above["radius"]).tolist() == [0, 0, 1]
    # why squares are not compared: at r = fl(sqrt(10)) the product r * r rounds above 10 = s
    assert exact["radius"] * exact["radius"] > 10.0 and not np.sqrt(np.float64(10.0)) < exact["radius"]


def test_x_zero_artefact():
    b, d = rf.x_zero(BOX), rf.x_zero(DISC)
    assert not brute(b["ref"], b["new"], 5.0, BOX).any()                 # nothing is near anything
    assert rn.dedup_box(b["ref"], b["new"], 5.0).tolist() == [0, 0, 1, 1, 1]
    assert rn.dedup_disc(d["ref"], d["new"], 5.0).tolist() == [1, 1, 1, 1, 1]
    empty = np.zeros((0, 2), np.float32)
    assert rn.dedup_box(empty, b["new"], 5.0).tolist() == [0, 0, 1, 1, 1]            # also with no reference point at all


@pytest.mark.parametrize("mode", [BOX, DISC])
def test_nan_points_are_kept(mode):
    c = rf.nan_points(mode)
    assert rn.dedup(c["ref"], c["new"], c["radius"], mode).tolist() == [1, 1, 1, 0, 1]


@pytest.mark.parametrize("mode", [BOX, DISC])
def test_listed_reference_points(mode):
    want = ([1, 0, 1, 0, 1, 1], [0, 1, 0, 1, 0, 1], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 1], [1, 1, 1, 1, 1, 1], [1, 1, 0, 1, 1, 1])
    for c, w in zip(rf.listed(mode), want):
        assert rn.dedup(c["ref"], c["new"], c["radius"], mode, c["ref_idx"]).tolist() == w, c["ref_idx"]
        inside = [j for j in c["ref_idx"] if 0 <= j < len(c["ref"])]
        assert rn.dedup(c["ref"], c["new"], c["radius"], mode, inside).tolist() == w


@pytest.mark.parametrize("mode", [BOX, DISC])
def test_last_point_of_the_last_tile_is_the_only_duplicate_maker(mode):
    c = rf.last_of_last_tile(mode)
    assert len(c["ref"]) == 2 * rf.T + 1 and len(c["new"]) == 257
    assert rn.dedup(c["ref"][:-1], c["new"], c["radius"], mode).all()
    keep = rn.dedup(c["ref"], c["new"], c["radius"], mode)
    assert np.flatnonzero(keep == 0).tolist() == [200]


@pytest.mark.parametrize("mode", [BOX, DISC])
def test_early_exit_fixture_settles_one_wave_and_keeps_another_busy(mode):
    c = rf.early_exit(mode)
    ref, new, r = c["ref"], c["new"], c["radius"]
    assert len(new) == rf.BLOCK and len(ref) == 2 * rf.T + 1
    first = rn.dedup(ref[:rf.T], new, r, mode)
    assert not first[:64].any() and first[64:].all()               # wave 0 is settled after tile 0, nobody else is
    assert rn.dedup(ref[:2 * rf.T], new, r, mode)[64:].all()       # tiles 0 and 1 settle nobody else
    keep = rn.dedup(ref, new, r, mode)
    assert np.flatnonzero(keep[64:] == 0).tolist() == [250 - 64]   # wave 3 needs the last tile


@pytest.mark.parametrize("mode", [BOX, DISC])
def test_replenish_restatement(mode):
    c = rf.replenish_case(150, 257, mode, 5)
    xy, xyz, n_dup, n_behind = rn.replenish(c["ref"], c["ref_xyz"], c["new"], c["new_xyz"], c["radius"], mode, c["Rt"])
    n_ref, n_new = 150, 257
    assert np.array_equal(xy[:n_ref], c["ref"]) and np.array_equal(xyz[:n_ref], c["ref_xyz"])
    assert n_dup + n_behind + (len(xy) - n_ref) == n_new and n_dup > 20 and n_behind > 20 and len(xy) - n_ref > 20
    keep = rn.dedup(c["ref"], c["new"], c["radius"], mode).astype(bool)
    moved = (c["Rt"][:, :3] @ c["new_xyz"].astype(np.float64).T).T + c["Rt"][:, 3]
    front = moved[:, 2].astype(np.float32) > 0
    assert np.array_equal(xy[n_ref:], c["new"][keep & front])
    assert np.allclose(xyz[n_ref:], moved[keep & front], rtol=1e-6, atol=1e-6) and (xyz[n_ref:, 2] > 0).all()
    # exactly one survivor of the filter lands on z == 0 and is dropped for it
    z = np.array([rn.move(c["Rt"], p)[2] for p in c["new_xyz"][keep]])
    assert (z == 0).sum() >= 1 and n_dup == int((~keep).sum()) and n_behind == int((z <= 0).sum())


def test_move_rounds_once():
    Rt = np.array([[1, 0, 0, 1e-9], [0, 1, 0, 0], [0.1, 0.2, 0.3, 0.7]])
    p = np.array([1.1, 2.2, 3.3], np.float32)
    x, y, z = (np.float64(v) for v in p)
    assert rn.move(Rt, p)[2] == np.float32(0.1 * x + 0.2 * y + 0.3 * z + 0.7)
    assert rn.move(Rt, p)[0] == np.float32(x + 0.0 * y + 0.0 * z + 1e-9)
