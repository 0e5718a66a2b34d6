"""The grey roles of pyramid.hip's base launch stage aligned dwords of the raw BGR rows (csrc/pyr_grey_plan.hip.h): grey frames
given as BGR from device pointers of all four alignment classes, inside a buffer of non-grey noise, at the widths around the first
interior tile of the raw launch (every misalignment of a raw row), on both sides of the tail guards and with interior tiles at
every level.  Every read-back -- levels, padded levels with every border byte, derivative words -- equals the integer numpy
definition of tests/pyr_numpy.py, the storage word says grey, a set of 32 mixed jobs equals the jobs' own launches, and all of it
equals the same calls under SVO_PYR_MONO_STORAGE=0.  The switch is read once per process, so both settings run `_child` in a
fresh process (this file, run as a script) and the tests compare what the children saved."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pyr_fixtures as pf  # noqa: E402
from test_gpu_pyr_mono_storage import _definition_bytes, _readbacks, _stored_word  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(w, h, lv) for w, h in ((129, 45), (130, 46), (131, 44), (132, 49), (133, 49), (135, 45)) for lv in (2, 4)] + \
         [(260, 66, 3), (516, 132, 4)]
KINDS = ("ramps", "random")
OFFSETS = (0, 1, 2, 3)
SET = (132, 49, 4)            # the geometry of the mixed set
GATED = (5, 22)           # a colour job into a grey-stored pyramid, a grey job into a colour-stored one
SETTINGS = {"default": {}, "storage0": {"SVO_PYR_MONO_STORAGE": "0"}}


def _grey(w, h, kind, seed=0):
    return pf.grey(pf.image(w, h, 3, kind, seed))


def _key(w, h, lv, kind, o):
    return f"{w}x{h}_L{lv}_{kind}_{o}"


def _set_image(k):
    """Job k of the mixed set: (image, byte offset of its device pointer, grey?)."""
    w, h, _ = SET
    img = _grey(w, h, KINDS[k % 2], seed=10 + k)
    if k % 3 == 2:  # one byte off grey, somewhere else per job
        img = img.copy()
        flat = img.reshape(-1)
        i = (k * 7919) % flat.size
        flat[i] = flat[i] + 1 if flat[i] < 255 else 254
    return img, k % 4, k % 3 != 2


def _set_previous(k):
    """What pyramid k of the mixed set held before it: colour for even k, grey for odd k."""
    w, h, _ = SET
    return pf.image(w, h, 3, "ramps", seed=40 + k) if k % 2 == 0 else _grey(w, h, "random", seed=40 + k)


class _Placed:
    """A device image at byte `offset` of a buffer of non-grey noise that is a little larger than the image."""

    def __init__(self, img, offset):
        import torch

        n = img.size
        noise = np.random.default_rng(n + offset).integers(0, 256, n + 64, dtype=np.uint8)
        noise[offset:offset + n] = np.ascontiguousarray(img).ravel()
        self.buf = torch.from_numpy(noise).cuda()
        self.ptr = self.buf.data_ptr() + offset
        assert self.ptr % 4 == offset


def _child(out):
    import torch

    torch.cuda.is_available()
    from ros_stereo_slam_amd import capi

    ctx = capi.Context(0)
    res = {}
    for w, h, lv in SHAPES:
        p = ctx.pyramid(w, h, 3, lv)
        for kind in KINDS:
            for o in OFFSETS:
                placed = _Placed(_grey(w, h, kind), o)
                p.build(placed.ptr, capi.MEM_DEVICE)
                ctx.sync()
                res["rb_" + _key(w, h, lv, kind, o)] = _readbacks(p)
                res["mono_" + _key(w, h, lv, kind, o)] = np.array(p.is_mono())
                res["stored_" + _key(w, h, lv, kind, o)] = _stored_word(ctx, p)
        p.close()
    # the mixed set of 32: grey at the four offsets, colour (one byte off grey), two jobs gated off
    w, h, lv = SET
    pyrs = [ctx.pyramid(w, h, 3, lv) for _ in range(32)]
    for k, q in enumerate(pyrs):
        q.build(np.ascontiguousarray(_set_previous(k)))
    placed = [_Placed(*_set_image(k)[:2]) for k in range(32)]
    shut = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.build_pyramids(pyrs, [x.ptr for x in placed], [shut if k in GATED else None for k in range(32)])
    ctx.sync()
    single = ctx.pyramid(w, h, 3, lv)
    for k, q in enumerate(pyrs):
        res[f"set_{k}"], res[f"setmono_{k}"], res[f"stored_set_{k}"] = _readbacks(q), np.array(q.is_mono()), _stored_word(ctx, q)
        single.build(placed[k].ptr, capi.MEM_DEVICE)
        ctx.sync()
        res[f"own_{k}"], res[f"ownmono_{k}"], res[f"stored_own_{k}"] = _readbacks(single), np.array(single.is_mono()), _stored_word(ctx, single)
        q.close()
    single.close()
    np.savez(out, **res)
    ctx.close()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("grey_staging")
    out = {}
    for name, env in SETTINGS.items():
        f = d / f"{name}.npz"
        r = subprocess.run([sys.executable, __file__, str(f)], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=300, cwd=str(ROOT))
        assert r.returncode == 0, name + ": " + r.stdout[-2000:] + r.stderr[-4000:]
        out[name] = dict(np.load(f))
    return out


@pytest.mark.parametrize("w,h,lv", SHAPES, ids=lambda v: str(v))
def test_read_backs_equal_the_definition_at_every_alignment(runs, w, h, lv):
    got = runs["default"]
    for kind in KINDS:
        want = _definition_bytes(_grey(w, h, kind), lv)
        for o in OFFSETS:
            key = _key(w, h, lv, kind, o)
            assert np.array_equal(got["rb_" + key], want), key
            assert int(got["stored_" + key]) == 1 and bool(got["mono_" + key]), key


def test_thirty_two_mixed_jobs_equal_their_own_launches(runs):
    got = runs["default"]
    for k in range(32):
        img, _, grey = _set_image(k)
        if k in GATED:  # previous bytes and words
            assert np.array_equal(got[f"set_{k}"], _definition_bytes(_set_previous(k), SET[2])), f"gated job {k}"
            assert int(got[f"stored_set_{k}"]) == (3 if k % 2 == 0 else 1) and bool(got[f"setmono_{k}"]) == (k % 2 == 1), f"gated job {k}"
            continue
        assert np.array_equal(got[f"set_{k}"], got[f"own_{k}"]), f"job {k} differs from its own launch"
        assert np.array_equal(got[f"set_{k}"], _definition_bytes(img, SET[2])), f"job {k}"
        assert int(got[f"stored_set_{k}"]) == int(got[f"stored_own_{k}"]) == (1 if grey else 3), f"job {k}"
        assert bool(got[f"setmono_{k}"]) == bool(got[f"ownmono_{k}"]) == grey, f"job {k}"


def test_storage_off_gives_the_same_read_backs(runs):
    ref, got = runs["storage0"], runs["default"]
    assert sorted(got) == sorted(ref)
    for k in ref:
        if k.startswith("stored_"):
            assert int(ref[k]) == 3, k
        else:
            assert np.array_equal(got[k], ref[k]), f"{k} differs from SVO_PYR_MONO_STORAGE=0"


if __name__ == "__main__":
    _child(sys.argv[1])
