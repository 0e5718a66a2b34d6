"""csrc/pyramid.hip at every seam of tests/pyr_fixtures.py, read back AS STORED: the levels, their reflect-101 borders (every
byte) and the packed Scharr derivative levels with their zero border, against the integer numpy definition of tests/pyr_numpy.py
-- from host and from device images (the latter ending directly in front of a sentinel band), over rebuilds of one pyramid, the
derivative-only launch, up to 32 gated pyramids in one set of launches (both kernel-argument layouts), and LK against the oracle
at the smallest legal images.  Exact equality of integers throughout.  tests/test_pyr_numpy.py shows on the CPU that the table
reaches every seam and that the definition agrees with the oracle."""
import ctypes as C

import numpy as np
import pytest

import pyr_fixtures as pf
import pyr_numpy as pn
from ros_stereo_slam_amd import capi, synth
from test_gpu_lk import _compare_lk

pytestmark = pytest.mark.gpu

GUARD = 64            # bytes of sentinel on either side of a device image
SENTINEL = 0xA5


def _has_words(c):
    return c in (1, 3)


def check_pyramid(pyr, d, what):
    """All three read-backs of every level against a Definition; C == 4 holds no derivative words and must say so."""
    for l in range(pyr.levels):
        diff = pn.where_differs(pyr.level(l), d.levels[l], 0, "level")
        assert diff is None, f"{what}: level {l}: {diff}"
        diff = pn.where_differs(pyr.padded_level(l), d.padded[l], pf.PYR_PAD, "padded")
        assert diff is None, f"{what}: padded level {l}: {diff}"
        if _has_words(pyr.c):
            diff = pn.where_differs(pyr.derivative_level(l), d.words[l], pf.DERIV_PAD, "deriv")
            assert diff is None, f"{what}: derivative level {l}: {diff}"
    if not _has_words(pyr.c):
        with pytest.raises(capi.SvoError) as err:
            pyr.derivative_level(0)
        assert err.value.code == capi.SVO_ERR_STATE


def snapshot(pyr):
    """Everything the three read-backs and the mono word show, as bytes."""
    parts = [pyr.padded_level(l).tobytes() for l in range(pyr.levels)]
    if _has_words(pyr.c):
        parts += [pyr.derivative_level(l).tobytes() for l in range(pyr.levels)]
    return b"".join(parts) + bytes([pyr.is_mono()])


class BandedImage:
    """A device image whose last byte lies directly in front of a sentinel band; `lead` more sentinel bytes in front of it."""

    def __init__(self, img, lead=GUARD):
        import torch

        self.n, self.lead = img.size, lead
        self.buf = torch.full((lead + self.n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.buf[lead:lead + self.n].copy_(torch.from_numpy(np.array(img, order="C").ravel()))
        self.ptr = self.buf.data_ptr() + lead
        torch.cuda.synchronize()

    def check(self, img, what):
        host = self.buf.cpu().numpy()
        assert (host[:self.lead] == SENTINEL).all() and (host[self.lead + self.n:] == SENTINEL).all(), (what, "a guard band was written")
        assert np.array_equal(host[self.lead:self.lead + self.n], img.ravel()), (what, "the image was written")


# ------------------------------------------------------------------------------------------------ 1. every entry
@pytest.mark.parametrize("e", pf.TABLE, ids=pf.entry_id)
def test_every_entry_from_host_and_device_images(ctx, e):
    host = ctx.pyramid(e.w, e.h, e.c, e.levels)
    dev = ctx.pyramid(e.w, e.h, e.c, e.levels)
    try:
        for kind in pf.IMAGE_KINDS:
            img = pf.image(e.w, e.h, e.c, kind)
            d = pf.definition(e.w, e.h, e.c, e.levels, kind)
            what = f"{pf.entry_id(e)} {kind}"
            check_pyramid(host.build(np.ascontiguousarray(img)), d, what + ", host image")
            # the device image starts at any byte alignment: its end is what the band fixes
            banded = BandedImage(img, lead=GUARD + pf.TABLE.index(e) % 4)
            dev.build(banded.ptr, capi.MEM_DEVICE)
            ctx.sync()
            banded.check(img, what)
            check_pyramid(dev, d, what + ", device image")
            assert snapshot(dev) == snapshot(host), what + ": device and host builds differ"
    finally:
        host.close()
        dev.close()


def test_one_level_without_derivatives_launches_nothing_to_finish(ctx):
    """levels == 1 and no derivative levels: the finishing launch has no role, so the word is never published (the comment in
    launch_finish) -- a grey 3-channel image does not report mono; level 0 and its border are complete all the same."""
    e = next(x for x in pf.TABLE if x.levels == 1 and x.c == 3)
    img = pf.grey(pf.image(e.w, e.h, e.c))
    with_deriv = ctx.pyramid(e.w, e.h, e.c, 1).build(np.ascontiguousarray(img))
    without = ctx.pyramid(e.w, e.h, e.c, 1, want_deriv=False).build(np.ascontiguousarray(img))
    try:
        assert with_deriv.is_mono() and not without.is_mono()
        d = pf.define(img, 1)
        check_pyramid(with_deriv, d, "one level, Scharr role only")
        assert pn.where_differs(without.padded_level(0), d.padded[0], pf.PYR_PAD, "padded") is None
        with pytest.raises(capi.SvoError) as err:
            without.derivative_level(0)
        assert err.value.code == capi.SVO_ERR_STATE
    finally:
        with_deriv.close()
        without.close()


# ------------------------------------------------------------------------------------------------ 2. rebuild
REBUILD = [e for e in pf.TABLE if (e.w, e.h) == (pf.MIN_SIDE, pf.MIN_SIDE) or pf._tail_last_fail(e)]
assert {e.c for e in REBUILD if e.w == pf.MIN_SIDE} == set(pf.CHANNELS) and {e.c for e in REBUILD if e.w > pf.MIN_SIDE} == set(pf.CHANNELS)


@pytest.mark.parametrize("e", REBUILD, ids=pf.entry_id)
def test_rebuild_leaves_nothing_of_the_image_before(ctx, e):
    a, b = pf.image(e.w, e.h, e.c, "ramps"), pf.image(e.w, e.h, e.c, "random", seed=1)
    used, fresh = ctx.pyramid(e.w, e.h, e.c, e.levels), ctx.pyramid(e.w, e.h, e.c, e.levels)
    try:
        used.build(np.ascontiguousarray(a))
        check_pyramid(used, pf.definition(e.w, e.h, e.c, e.levels, "ramps"), "first image")
        used.build(np.ascontiguousarray(b))
        fresh.build(np.ascontiguousarray(b))
        check_pyramid(used, pf.definition(e.w, e.h, e.c, e.levels, "random", 1), "second image in a used pyramid")
        assert snapshot(used) == snapshot(fresh)
    finally:
        used.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------ 3. derivative-only launch
def _lk_points(w, h, n=300, seed=5):
    return np.random.default_rng(seed).uniform([-15, -15], [w + 15, h + 15], (n, 2)).astype(np.float32)


@pytest.mark.parametrize("w,h,c,grey", [(45, 47, 1, False), (45, 47, 3, False), (45, 47, 3, True), (133, 49, 3, False), (137, 49, 1, False)])
def test_derivative_only_launch(ctx, w, h, c, grey):
    """A pyramid created without derivative levels holds none after a build; the tracker derives them when the pyramid is its
    first image (svo_build_derivatives, publish == 0), which must neither clear nor republish the mono word; the next build
    drops them again."""
    a, b = pf.image(w, h, c, "ramps"), pf.image(w, h, c, "random", seed=2)
    if grey:
        a, b = pf.grey(a), pf.grey(b)
    pts = _lk_points(w, h)
    lazy = ctx.pyramid(w, h, c, 4, want_deriv=False)
    eager, nxt = ctx.pyramid(w, h, c, 4), ctx.pyramid(w, h, c, 4).build(np.ascontiguousarray(b))
    try:
        for img in (a, b):
            img = np.ascontiguousarray(img)
            lazy.build(img)
            eager.build(img)
            d = pf.define(img, 4)
            for l in range(4):
                with pytest.raises(capi.SvoError) as err:
                    lazy.derivative_level(l)
                assert err.value.code == capi.SVO_ERR_STATE
                assert pn.where_differs(lazy.padded_level(l), d.padded[l], pf.PYR_PAD, "padded") is None
            mono = lazy.is_mono()
            assert mono == (c == 3 and grey) and eager.is_mono() == mono
            got, want = ctx.lk_track(lazy, nxt, pts), ctx.lk_track(eager, nxt, pts)
            assert all(np.array_equal(g.view(np.uint8), w_.view(np.uint8)) for g, w_ in zip(got, want))
            assert lazy.is_mono() == mono, "the derivative-only launch touched the mono word"
            check_pyramid(lazy, d, "derived on demand")
            check_pyramid(eager, d, "derived at the build")
    finally:
        lazy.close()
        eager.close()
        nxt.close()


# ------------------------------------------------------------------------------------------------ 4. many pyramids, gated
MANY = [(k, c, (45, 47, 4)) for k in (1, 2, 3, 32) for c in pf.CHANNELS] + [(3, 1, (130, 46, 3)), (32, 3, (130, 46, 3)), (2, 4, (129, 45, 2))]
assert all(pf.Entry(w, h, c, lv) in pf.TABLE for _, c, (w, h, lv) in MANY)


def _many_images(w, h, c, k):
    """k images for the build under test (all with colour) and k different ones built before it (every other one grey)."""
    new = [pf.image(w, h, c, "random", seed=100 + a) for a in range(k)]
    old = [pf.image(w, h, c, "ramps" if a % 2 else "random", seed=200 + a) for a in range(k)]
    old = [pf.grey(x) if a % 2 == 0 else x for a, x in enumerate(old)]
    return new, old


@pytest.mark.parametrize("k,c,geom", MANY, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_many_pyramids_in_one_set_of_launches(ctx, k, c, geom):
    import torch

    w, h, levels = geom
    new, old = _many_images(w, h, c, k)
    d_new, d_old = [pf.define(x, levels) for x in new], [pf.define(x, levels) for x in old]
    dev_new, dev_old = [BandedImage(x) for x in new], [BandedImage(x) for x in old]
    pyrs = [ctx.pyramid(w, h, c, levels) for _ in range(k)]
    single = ctx.pyramid(w, h, c, levels)
    shut, open_ = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        # no gates at all: every job builds its own image
        ctx.build_pyramids(pyrs, [x.ptr for x in dev_old])
        ctx.sync()
        for a, p in enumerate(pyrs):
            check_pyramid(p, d_old[a], f"k = {k}, no gates, job {a}")
            assert p.is_mono() == (c == 3 and a % 2 == 0), (k, a)
        before = [snapshot(p) for p in pyrs]
        # gates: 0, 1, NULL, 0, 1, NULL, ...
        gates = [(shut, open_, None)[a % 3] for a in range(k)]
        ctx.build_pyramids(pyrs, [x.ptr for x in dev_new], gates)
        ctx.sync()
        for a, p in enumerate(pyrs):
            if a % 3 == 0:
                assert snapshot(p) == before[a], f"k = {k}: job {a} was shut and changed"
                check_pyramid(p, d_old[a], f"k = {k}, shut job {a}")
            else:
                check_pyramid(p, d_new[a], f"k = {k}, open job {a}")
                assert not p.is_mono()
                assert snapshot(p) == snapshot(single.build(np.ascontiguousarray(new[a]))), f"k = {k}: job {a} differs from its single build"
        for a in range(k):
            dev_new[a].check(new[a], ("new", k, a))
            dev_old[a].check(old[a], ("old", k, a))
    finally:
        for p in pyrs + [single]:
            p.close()


def test_too_many_pyramids_and_mixed_geometry_are_refused_and_launch_nothing(ctx):
    w, h, c, levels = 45, 47, 3, 4
    img = pf.image(w, h, c)
    other = BandedImage(pf.image(w, h, c, "ramps"))
    pyrs = [ctx.pyramid(w, h, c, levels).build(np.ascontiguousarray(img)) for _ in range(pf.PYR_JOBS + 1)]
    odd = [ctx.pyramid(47, 45, c, levels), ctx.pyramid(w, h, 1, levels), ctx.pyramid(w, h, c, 3)]
    try:
        before = [snapshot(p) for p in pyrs[:3]]
        with pytest.raises(capi.SvoError) as err:
            ctx.build_pyramids(pyrs, [other.ptr] * len(pyrs))
        assert err.value.code == capi.SVO_ERR_ARG
        for o in odd:
            with pytest.raises(capi.SvoError) as err:
                ctx.build_pyramids([pyrs[0], pyrs[1], o], [other.ptr] * 3)
            assert err.value.code == capi.SVO_ERR_ARG
        P = C.c_void_p * 1
        assert ctx.lib.svo_pyramid_build_many(ctx._h, 0, P(pyrs[0]._h.value), P(other.ptr), None) == capi.SVO_ERR_ARG
        assert ctx.lib.svo_pyramid_build_many(ctx._h, 1, P(pyrs[0]._h.value), P(0), None) == capi.SVO_ERR_ARG
        ctx.sync()
        assert [snapshot(p) for p in pyrs[:3]] == before
        ctx.build_pyramids(pyrs[:pf.PYR_JOBS], [other.ptr] * pf.PYR_JOBS)       # 32 is the most, and is accepted
        ctx.sync()
        assert snapshot(pyrs[pf.PYR_JOBS - 1]) != before[0] and snapshot(pyrs[pf.PYR_JOBS]) == before[0]
    finally:
        for p in pyrs + odd:
            p.close()


# ------------------------------------------------------------------------------------------------ 5. LK at the smallest sizes
@pytest.mark.parametrize("c,colour", [(1, False), (3, False), (3, True)], ids=["c1", "c3-grey", "c3-colour"])
@pytest.mark.parametrize("w,h", [(44, 44), (45, 47), (131, 97), (129, 49)])
def test_lk_at_small_sizes_equals_the_oracle(ctx, orc, w, h, c, colour):
    """Status, points, err and minEig bit for bit where level 3 is as small as 6 x 6 and every window reaches into a border
    that has folded more than once; points from 15 pixels outside the image on one side to 15 outside on the other."""
    a, b = synth.textured_pair(w, h, c, shift=(1.0, 0.5), seed=9, colour=colour)
    pts = _lk_points(w, h)
    _, st = _compare_lk(ctx, orc, a, b, pts)
    assert 0 < int(st.sum()) < len(pts), "both statuses must occur"
