"""The finish of the F-matrix RANSAC -- mask, compaction of the payload, counts -- through ``svo_fransac_batch``, the device-pointer
entry of the launch sequence the lock-step front-ends queue (``fransac.hip``: a problem whose loop ends in the first 64
iterations is finished by all waves of the second launch from the winner's bit plane; every other problem by the workgroup
with the last ticket).

The comparator of every case is the library's own lone ``svo_fransac`` (host form) on the same pairs and seed: mask, model,
inlier count and iterations run are equal bit for bit, the mask's tail up to the capacity is zero, and the compacted arrays are
numpy's ``payload[mask == 1]``; rows of the outputs behind the kept ones are left as they were.  No tolerance anywhere.

A payload array whose output pointer equals its input pointer is NOT permitted, before this finish or with it: a kept row's
destination is an earlier row that another lane (with the wide finish: another workgroup) may not have read yet
(``fransac.hip``'s header, ``include/svo.h``).  There is no such case here."""
import ctypes as C

import numpy as np
import pytest

from geom_fixtures import two_view

pytestmark = pytest.mark.gpu

SENTINEL = 0xCC          # what the mask holds before a call
ROW_SENTINEL = -12345.0  # ... and the payload outputs


def pairs(n, inliers, seed):
    """n correspondences of a moving camera, `inliers` of them consistent; collinear: every point on one image line."""
    if inliers == "collinear":
        t = np.linspace(10.0, 600.0, n)
        x1 = np.stack([t, 0.5 * t + 20.0], 1).astype(np.float32)
        return x1, (x1 + np.float32(3.0)).astype(np.float32)
    if inliers == "noise":
        rng = np.random.default_rng(seed)
        return (rng.uniform(0, 600, (n, 2)).astype(np.float32), rng.uniform(0, 600, (n, 2)).astype(np.float32))
    x1, x2, *_ = two_view(n=n, n_out=n - int(round(n * inliers)), seed=seed, noise=0.15)
    return x1, x2


class Problem:
    """One problem on the device, its outputs pre-filled so that what a call leaves alone can be told from what it wrote."""

    def __init__(self, n, cap=None, inliers=0.85, seed=1, skew=0, strides=(2, 3), thr=1.0, max_iters=1000, gate=None,
                 odd_payload=False):
        import torch

        self.n, self.cap, self.thr, self.max_iters, self.seed = n, cap or n, thr, max_iters, seed
        cap = self.cap
        self.x1, self.x2 = pairs(n, inliers, seed)
        rng = np.random.default_rng(900 + seed + n)
        dev = "cuda"

        def points(x):
            full = rng.uniform(0, 600, (cap + skew, 2)).astype(np.float32)  # live-looking values behind the live count
            full[skew:skew + n] = x
            return torch.from_numpy(full).to(dev)

        self._p1, self._p2 = points(self.x1), points(self.x2)
        self.p1, self.p2 = self._p1[skew:], self._p2[skew:]
        assert self.p1.data_ptr() % 16 == (8 if skew else 0)
        self.d_n = torch.tensor([n], dtype=torch.int32, device=dev) if cap > n else None
        self.mask = torch.full((cap,), SENTINEL, dtype=torch.uint8, device=dev)
        self.F9 = torch.full((9,), float("nan"), dtype=torch.float64, device=dev)
        self.ints = torch.full((3,), -7, dtype=torch.int32, device=dev)  # inlier count, iterations run, payload count
        self.payload, self.ins, self.outs = [], [], []
        for s in strides:
            host = rng.normal(size=(cap, s)).astype(np.float32)
            off = 1 if (odd_payload and s == 2) else 0  # rows of two floats that are only 4-byte aligned
            src = torch.zeros(cap * s + off, dtype=torch.float32, device=dev)
            src[off:] = torch.from_numpy(host.reshape(-1)).to(dev)
            dst = torch.full((cap * s + off,), ROW_SENTINEL, dtype=torch.float32, device=dev)
            self.payload.append(host)
            self.ins.append(src[off:])
            self.outs.append(dst[off:])
        self.gate = None if gate is None else torch.tensor([gate], dtype=torch.int32, device=dev)

    def as_dict(self):
        ints = self.ints.data_ptr()
        d = dict(p1=self.p1, p2=self.p2, cap=self.cap, d_n=self.d_n, threshold=self.thr, max_iters=self.max_iters,
                 seed=self.seed, mask=self.mask, F9=self.F9, inlier_count=ints, iters_run=ints + 4,
                 payload=[(i, h.shape[1], o) for i, h, o in zip(self.ins, self.payload, self.outs)], gate=self.gate)
        if self.payload:
            d["payload_count"] = ints + 8
        return d

    def lone(self, ctx):
        """count, mask, model, iterations of the lone svo_fransac on the live pairs."""
        return ctx.fransac(self.x1, self.x2, self.thr, 0.99, self.max_iters, seed=self.seed)

    def check(self, ctx, want=None):
        cnt, mask, F, iters = want or self.lone(ctx)
        got_mask = self.mask.cpu().numpy()
        ints = self.ints.cpu().numpy()
        assert (int(ints[0]), int(ints[1])) == (cnt, iters), (self.n, ints, cnt, iters)
        assert np.array_equal(got_mask[:self.n], mask), (self.n, np.flatnonzero(got_mask[:self.n] != mask)[:8])
        assert not got_mask[self.n:].any(), "the mask's tail up to the capacity must be zero"
        assert np.array_equal(self.F9.cpu().numpy().reshape(3, 3), F)
        assert int(mask.sum()) == cnt
        if self.payload:
            assert int(ints[2]) == cnt
        for host, out in zip(self.payload, self.outs):
            got = out.cpu().numpy().reshape(self.cap, -1)
            assert np.array_equal(got[:cnt], host[:self.n][mask == 1])
            assert (got[cnt:] == np.float32(ROW_SENTINEL)).all(), "rows behind the kept ones were written"
        return cnt, iters

    def check_untouched(self):
        assert (self.mask.cpu().numpy() == SENTINEL).all()
        assert (self.ints.cpu().numpy() == -7).all() and np.isnan(self.F9.cpu().numpy()).all()
        for out in self.outs:
            assert (out.cpu().numpy() == np.float32(ROW_SENTINEL)).all()


def run(ctx, problems):
    import torch

    torch.cuda.synchronize()
    ctx.fransac_batch([p.as_dict() for p in problems])
    ctx.sync()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n", [15, 63, 64, 65, 255, 256, 257, 1030])
def test_pair_counts_around_the_blocks_of_the_finish(ctx, n, k):
    """64: a block of the wide finish (a pair per lane); 256: a step of the scoring pass, four words of the bit plane;
    1 030: five steps and seventeen blocks, each with the popcounts of the steps before it as its prefix.  With one problem
    the lone-chunk build runs (four waves a workgroup, a block per wave), with two the single-wave build."""
    ps = [Problem(n, seed=n)] + ([Problem(300, seed=n + 1)] if k == 2 else [])
    run(ctx, ps)
    res = [p.check(ctx) for p in ps]
    assert res[0][1] <= 64  # the loop ended in the first phase: the second launch's waves finished it


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n,cap,skew", [(257, 263, 0), (1030, 1101, 1), (255, 255, 1), (64, 1030, 0), (1030, 1030, 0)])
def test_capacity_live_count_and_alignment(ctx, n, cap, skew, k):
    """cap > n with the live count on the device (the tail of the mask is zero, whole blocks of it beyond n included), a
    capacity that is no multiple of four, and pairs that are only 8-byte aligned (the scoring pass takes single pairs)."""
    ps = [Problem(n, cap=cap, skew=skew, seed=3 * n + cap) for _ in range(k)]
    run(ctx, ps)
    for p in ps:
        p.check(ctx)


@pytest.mark.parametrize("n,k", [(4428, 2), (4428, 1), (16500, 1)])
def test_second_trips_of_the_finish(ctx, n, k):
    """4 428 (the lattice of the benchmark): 70 blocks over the 64 single-wave workgroups and 68 words before the last step,
    so a workgroup's second block and a lane's second word of the prefix; 16 500: the same for the lone-chunk build's 256 waves."""
    ps = [Problem(n, seed=n + j, inliers=0.8) for j in range(k)]
    run(ctx, ps)
    for p in ps:
        assert p.check(ctx)[1] <= 64


@pytest.mark.parametrize("strides,odd",[((), False), ((2,), False), ((2, 3, 1), False), ((2, 3), True)])
def test_payload_strides(ctx, strides, odd):
    """none, one array of rows of two, rows of two + three + one together; rows of two that are only 4-byte aligned."""
    ps = [Problem(1030, cap=1040, strides=strides, seed=21, odd_payload=odd), Problem(257, strides=strides, seed=22, odd_payload=odd)]
    run(ctx, ps)
    for p in ps:
        p.check(ctx)


def mixed_sixteen():
    ps = []
    for a in range(16):
        kind = a % 5
        if kind == 0:
            ps.append(Problem(1030 + a, cap=1100, inliers=0.85, seed=40 + a))                  # ends in the first phase
        elif kind == 1:
            ps.append(Problem(600 + a, inliers=0.30, seed=40 + a))                             # runs to max_iters
        elif kind == 2:
            ps.append(Problem(200 + a, inliers="noise", max_iters=64, seed=40 + a, thr=0.05))  # pure noise, 64 iterations
        elif kind == 3:
            ps.append(Problem(8 + (a % 7), seed=40 + a, inliers=1.0))                          # 8 .. 14 pairs: least median
        else:
            ps.append(Problem(40 + a, inliers="collinear", seed=40 + a))                       # no sample can be drawn
    return ps


def test_sixteen_problems_of_every_kind_in_one_launch(ctx):
    ps = mixed_sixteen()
    run(ctx, ps)
    res = [p.check(ctx) for p in ps]
    for a, (cnt, iters) in enumerate(res):
        if a % 5 == 0:
            assert 0 < iters <= 64 and cnt > 0, "this job is meant to end in the first phase, with a model"
        if a % 5 == 1:
            assert iters == 1000, "the low-inlier job is meant to run the second phase to its end"
        if a % 5 == 4:
            assert cnt == 0


def test_a_call_of_at_most_64_iterations(ctx):
    ps = [Problem(1030, max_iters=50, seed=61), Problem(65, max_iters=64, seed=62), Problem(12, max_iters=64, seed=63, inliers=1.0)]
    run(ctx, ps)
    for p in ps:
        p.check(ctx)
    one = [Problem(257, max_iters=20, seed=64)]
    run(ctx, one)
    one[0].check(ctx)


def test_closed_gate_leaves_one_job_alone_and_the_tickets_at_rest(ctx):
    import torch

    ps = [Problem(1030, seed=71, gate=1), Problem(257, seed=72, gate=0), Problem(600, inliers=0.3, seed=73),
          Problem(10, seed=74, gate=0, inliers=1.0)]
    want = [p.lone(ctx) for p in ps]
    run(ctx, ps)
    ps[1].check_untouched()
    ps[3].check_untouched()
    ps[0].check(ctx, want[0])
    ps[2].check(ctx, want[2])
    # the counters of the "last workgroup" hand-over are at rest, and an ordinary call gives its usual answer
    tickets = (C.c_uint * 2)(7, 7)
    dmask = torch.zeros(ps[0].n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.lib.svo_selftest_fransac_gate(ctx._h, C.c_void_p(ps[0].p1.data_ptr()), C.c_void_p(ps[0].p2.data_ptr()), ps[0].n,
                                             C.c_double(1.0), C.c_uint64(71), 1, C.c_void_p(dmask.data_ptr()), tickets) == 0
    assert tickets[0] == 0 and tickets[1] == 0
    again = [Problem(1030, seed=71), Problem(257, seed=72)]
    run(ctx, again)
    again[0].check(ctx, want[0])
    again[1].check(ctx, want[1])
    after = ps[0].lone(ctx)
    assert after[0] == want[0][0] and after[3] == want[0][3] and np.array_equal(after[1], want[0][1])


def test_two_calls_in_a_row_with_different_counts(ctx):
    """stale bit planes or a stale "finish pending" mark of the first call would show in the second, and the other way round"""
    first = [Problem(1030, seed=81), Problem(600, inliers=0.3, seed=82)]
    second = [Problem(257, seed=83), Problem(70, seed=84)]
    third = [Problem(12, seed=85, inliers=1.0), Problem(1030, cap=1100, seed=86)]
    for ps in (first, second, third):
        run(ctx, ps)
    for ps in (first, second, third):
        for p in ps:
            p.check(ctx)
