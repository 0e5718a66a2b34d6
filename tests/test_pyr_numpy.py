"""CPU side of the pyramid's seam tests: the numpy definition (tests/pyr_numpy.py) against the oracle at every entry of the seam
table, the loop form of reflect-101 against a walk, and the proof that the table of tests/pyr_fixtures.py reaches every seam of
csrc/pyramid.hip for every channel count the seam applies to -- so that tests/test_gpu_pyramid_seams.py cannot pass vacuously."""
import numpy as np
import pytest

import lk_numpy
import pyr_fixtures as pf
import pyr_numpy as pn


def _walk(idx, n):
    """Where |idx| steps from pixel 0 end when every step that would leave 0 .. n-1 turns round first."""
    if n == 1:
        return 0
    pos, d = 0, 1 if idx >= 0 else -1
    for _ in range(abs(idx)):
        if not 0 <= pos + d < n:
            d = -d
        pos += d
    return pos


def test_reflect101_loop_form_against_a_walk():
    for n in range(1, 9):
        idx = np.arange(-40, n + 41)
        got = pn.reflect101(idx, n)
        want = np.array([_walk(int(i), n) for i in idx])
        assert np.array_equal(got, want), (n, idx[got != want][:5])
        assert got.min() >= 0 and got.max() <= n - 1


def test_reflect101_differs_from_a_single_fold_where_the_border_is_wider_than_the_level():
    """What the loop form is for: a 32-pixel border round a 6-pixel level.  Inside one fold's reach the two agree."""
    idx = np.arange(-pf.PYR_PAD, 6 + pf.PYR_PAD)
    once = lk_numpy._reflect101(idx, 6)
    assert ((once < 0) | (once >= 6)).any()
    near = np.arange(-5, 11)
    assert np.array_equal(pn.reflect101(near, 6), lk_numpy._reflect101(near, 6))


@pytest.mark.parametrize("e", pf.TABLE, ids=pf.entry_id)
def test_definition_equals_the_oracle_at_every_entry(orc, e):
    for kind in pf.IMAGE_KINDS:
        d = pf.definition(e.w, e.h, e.c, e.levels, kind)
        assert [x.shape[:2] for x in d.levels] == [(h, w) for w, h in pf.level_sizes(e)]
        for l, lv in enumerate(d.levels):
            if l + 1 < e.levels:
                assert np.array_equal(orc.pyr_down(lv), d.levels[l + 1]), (kind, "pyr_down of level", l)
            dx, dy = lk_numpy.scharr(lv)
            ref = orc.scharr(lv)                                   # (h, w, c, 2) int16, unscaled
            assert np.array_equal(ref[..., 0], dx) and np.array_equal(ref[..., 1], dy), (kind, "scharr of level", l)
            assert d.padded[l].shape == (lv.shape[0] + 2 * pf.PYR_PAD, lv.shape[1] + 2 * pf.PYR_PAD, e.c)
            assert np.array_equal(d.padded[l][pf.PYR_PAD:-pf.PYR_PAD, pf.PYR_PAD:-pf.PYR_PAD], lv)
            if d.words is not None:
                p = pf.DERIV_PAD
                wx, wy = pn.unpack_words(d.words[l])
                assert np.array_equal(wx[p:-p, p:-p], 4 * dx) and np.array_equal(wy[p:-p, p:-p], 4 * dy), (kind, "packing of level", l)
                border = d.words[l].copy()
                border[p:-p, p:-p] = 0
                assert not border.any()


def test_padding_mirrors_about_the_edge_pixels():
    """`padded` on the ramps image: the pixel k outside an edge is the pixel k inside it, and the corner regions mirror both ways."""
    img = pf.image(45, 47, 3, "ramps")
    p = pn.padded(img, 10)
    for k in range(1, 11):
        assert np.array_equal(p[10 - k, 10:-10], img[k]) and np.array_equal(p[10 + 46 + k, 10:-10], img[46 - k])
        assert np.array_equal(p[10:-10, 10 - k], img[:, k]) and np.array_equal(p[10:-10, 10 + 44 + k], img[:, 44 - k])
    assert np.array_equal(p[7, 6], img[3, 4]) and np.array_equal(p[10 + 46 + 2, 10 + 44 + 5], img[44, 39])


def test_every_seam_is_reached(capsys):
    """Every seam of csrc/pyramid.hip, for every channel count it applies to, is hit by at least one entry of the table."""
    reach = pf.reach()
    missing = []
    with capsys.disabled():
        print()
        for s in pf.SEAMS:
            for c in s.channels:
                hit = reach[s.name][c]
                print(f"  {s.name} [c = {c}] ({s.source}): {', '.join(pf.entry_id(e) for e in hit) or 'NOT REACHED'}")
                if not hit:
                    missing.append((s.name, c))
    assert not missing, f"the seam table reaches none of: {missing}"
    assert {e.c for e in pf.TABLE} == set(pf.CHANNELS) and {e.levels for e in pf.TABLE} == {1, 2, 3, 4}


def test_the_tail_guard_widths_follow_from_the_kernel_constants():
    """Tile (1, 2) of a 49-row image is the one whose last staged row is the image's last: the predicate finds, per channel
    count, one width at which the guard alone denies the aligned path and the next at which it no longer does -- and at 129
    pixels, the first width at which the tile lies inside the image, it is still denied."""
    for c in pf.CHANNELS:
        fail = [w for w in range(129, 160) if pf._tail_last_fail(pf.Entry(w, 49, c, 4))]
        ok = [w for w in range(129, 160) if pf._tail_first_pass(pf.Entry(w, 49, c, 4))]
        assert len(fail) == 1 and ok == [fail[0] + 1], (c, fail, ok)
        assert pf.Entry(fail[0], 49, c, 4) in pf.TABLE and pf.Entry(ok[0], 49, c, 4) in pf.TABLE, (c, fail, ok)
        assert (1, 2, False) in pf._tail_tiles(129, 49, c)
