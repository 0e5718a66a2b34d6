"""ctypes binding of ``libsvo_hip.so`` (``include/svo.h``).

The shared library is the product; this module is plumbing.  It never falls back to a CPU
implementation: if the library is missing it raises, and ``Context()`` raises when no
gfx950 device is present.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import pathlib
import re
import weakref

import numpy as np

_HERE = pathlib.Path(__file__).resolve().parent
LIB_PATH = _HERE / "libsvo_hip.so"
HEADER_PATH = _HERE.parent / "include" / "svo.h"

SVO_OK = 0
SVO_ERR_ARG = -1
SVO_ERR_HIP = -2
SVO_ERR_CAPACITY = -3
SVO_ERR_NO_DEVICE = -4
SVO_ERR_TRACKING_LOST = -5
SVO_ERR_STATE = -6
MEM_HOST, MEM_DEVICE = 0, 1
K_PYRAMID, K_LK, K_FRANSAC, K_TRIANGULATE, K_PNP, K_POSEGRAPH, K_ANMS, K_BRIEF_INTEGRAL, K_BRIEF_DESCRIBE = range(9)
PG_ROBUST_NONE, PG_ROBUST_HUBER, PG_ROBUST_CAUCHY, PG_ROBUST_DCS, PG_ROBUST_GEMAN_MCCLURE = range(5)


class SvoError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libsvo_hip error {code}: {msg}")
        self.code = code


_lib = None


def declared_symbols() -> list[str]:
    """Every function ``include/svo.h`` declares (used by the export test)."""
    text = HEADER_PATH.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(svo_[a-z0-9_]+)\s*\(", text)))


def load() -> C.CDLL:
    """Load the library (building nothing).  Raises if it is absent -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    # SVO_LIB=<path>: an A/B variant build (tools/ab.sh) is loaded INSTEAD of the installed library, which is
    # never overwritten; the override must name an existing file (no silent fall-through to the default)
    path = pathlib.Path(os.environ["SVO_LIB"]) if os.environ.get("SVO_LIB") else LIB_PATH
    if not path.exists():
        raise ImportError(
            f"{path} is missing: build it with `make -C ros_stereo_slam_amd/csrc` "
            "(or __graft_entry__.build()); the HIP path has no CPU fallback")
    lib = C.CDLL(os.fspath(path))
    lib.svo_last_error.restype = C.c_char_p
    lib.svo_ctx_stream.restype = C.c_void_p
    _lib = lib
    return lib


def _check(rc: int):
    if rc != SVO_OK:
        raise SvoError(rc, load().svo_last_error().decode(errors="replace"))


def _ptr(a):
    """Pointer of a numpy array (host) or an int / object with data_ptr() (device)."""
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return C.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(int(a))


def _is_device(a) -> bool:
    return hasattr(a, "is_cuda") and bool(a.is_cuda)


def _mem_of(dev) -> int:
    return MEM_DEVICE if dev else MEM_HOST


def _image_shape(im):
    h, w = im.shape[:2]
    return w, h, (1 if im.ndim == 2 else im.shape[2])


def _make_params(cls, default_fn_name, overrides, *before):
    """A ``cls`` that the library's ``default_fn_name(*before, &p)`` filled, then the overrides by field name."""
    p = cls()
    getattr(load(), default_fn_name)(*before, C.byref(p))
    for k, v in overrides.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _as_params(cls, maker, value):
    """``value`` when it is a ``cls``; otherwise ``maker``'s struct with the overrides of a dict (None: the defaults)."""
    return value if isinstance(value, cls) else maker(**(value or {}))


def _known_fields(cls, c_name, names):
    """The parameter structs that refuse an unknown field with a TypeError rather than an assertion."""
    for k in names:
        if k not in dict(cls._fields_):
            raise TypeError(f"{c_name} has no field {k}")


class _Handle:
    """A library object a context owns: ``close()`` destroys it once, and only while the context still has its handle.  A
    subclass names the destroy function and says whether it is called as ``destroy(ctx, handle)`` or ``destroy(handle)``."""
    _destroy = None
    _destroy_takes_ctx = False

    def close(self):
        if self._h and self.ctx._h:
            destroy = getattr(self.ctx.lib, self._destroy)
            if self._destroy_takes_ctx:
                destroy(self.ctx._h, self._h)
            else:
                destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pyramid(_Handle):
    _destroy, _destroy_takes_ctx = "svo_pyramid_destroy", True

    def __init__(self, ctx: "Context", w: int, h: int, c: int, levels: int = 4, want_deriv: bool = True):
        """``want_deriv=False``: a pyramid without Scharr derivative levels (``svo_pyramid_create2``), as the front-end keeps
        for its right images; the tracker derives them when such a pyramid becomes its first image after all."""
        self.ctx, self.w, self.h, self.c, self.levels = ctx, w, h, c, levels
        self._h = C.c_void_p()
        _check(ctx.lib.svo_pyramid_create2(ctx._h, w, h, c, levels, int(bool(want_deriv)), C.byref(self._h)))
        ctx._children.add(self)

    def build(self, image, mem: int = MEM_HOST):
        if isinstance(image, np.ndarray):
            assert image.dtype == np.uint8 and image.shape == (self.h, self.w, self.c)
        _check(self.ctx.lib.svo_pyramid_build(self.ctx._h, self._h, _ptr(image), mem))
        return self

    def build_gated(self, d_image, d_gate):
        """Build from a device image unless the device int ``d_gate`` is 0 (``svo_pyramid_build_gated``); asynchronous."""
        _check(self.ctx.lib.svo_pyramid_build_gated(self.ctx._h, self._h, _ptr(d_image), _ptr(d_gate)))
        return self

    def is_mono(self) -> bool:
        """True when the image of the last build had B == G == R in every pixel (3-channel pyramids only)."""
        out = C.c_int()
        _check(self.ctx.lib.svo_pyramid_is_mono(self.ctx._h, self._h, C.byref(out)))
        return bool(out.value)

    def level(self, l: int) -> np.ndarray:
        w, h = C.c_int(), C.c_int()
        _check(self.ctx.lib.svo_pyramid_get_level(self.ctx._h, self._h, l, None, MEM_HOST,
                                                  C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, self.c), np.uint8)
        _check(self.ctx.lib.svo_pyramid_get_level(self.ctx._h, self._h, l, _ptr(out), MEM_HOST,
                                                  C.byref(w), C.byref(h)))
        return out

    def padded_level(self, l: int) -> np.ndarray:
        """Level ``l`` as stored, with its reflect-101 border: ``(h + 64, w + 64, c)`` uint8."""
        w, h = C.c_int(), C.c_int()
        _check(self.ctx.lib.svo_pyramid_get_padded_level(self.ctx._h, self._h, l, None, MEM_HOST, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, self.c), np.uint8)
        _check(self.ctx.lib.svo_pyramid_get_padded_level(self.ctx._h, self._h, l, _ptr(out), MEM_HOST, C.byref(w), C.byref(h)))
        return out

    def derivative_level(self, l: int) -> np.ndarray:
        """The packed Scharr words ``(4 dx & 0xffff) | (4 dy << 16)`` of level ``l`` with their zero border:
        ``(h + 64, w + 64, c)`` int32.  Raises ``SvoError`` (``SVO_ERR_STATE``) when the pyramid holds none."""
        w, h = C.c_int(), C.c_int()
        _check(self.ctx.lib.svo_pyramid_get_derivative_level(self.ctx._h, self._h, l, None, MEM_HOST, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, self.c), np.int32)
        _check(self.ctx.lib.svo_pyramid_get_derivative_level(self.ctx._h, self._h, l, _ptr(out), MEM_HOST, C.byref(w),
                                                             C.byref(h)))
        return out


class Context:
    """One per device: owns the HIP stream, scratch and kernel timers (``svo_ctx``)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        self._h = C.c_void_p()
        self._children = weakref.WeakSet()  # pyramids / front-ends that must go before the context
        _check(self.lib.svo_ctx_create(device, C.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            for child in list(self._children):
                child.close()
            self.lib.svo_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(self.lib.svo_ctx_sync(self._h))

    @property
    def stream(self) -> int:
        return self.lib.svo_ctx_stream(self._h)

    def enable_kernel_timing(self, on: bool = True):
        _check(self.lib.svo_ctx_enable_kernel_timing(self._h, int(on)))

    def reset_kernel_time(self):
        _check(self.lib.svo_ctx_reset_kernel_time(self._h))

    def kernel_time(self, kid: int):
        ms, n = C.c_double(), C.c_int()
        _check(self.lib.svo_ctx_kernel_time(self._h, kid, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- hot-path entry points (host-array convenience forms) ----
    def pyramid(self, w, h, c, levels=4, want_deriv=True) -> Pyramid:
        return Pyramid(self, w, h, c, levels, want_deriv)

    def build_pyramids(self, pyrs, d_images, d_gates=None):
        """``svo_pyramid_build_many``: up to 32 pyramids of one geometry from as many device images in one set of launches.
        ``d_gates``: None, or one entry per pyramid, each None or a device int (0 leaves that pyramid as it was).
        Asynchronous on the ctx stream."""
        k = len(pyrs)
        assert len(d_images) == k and (d_gates is None or len(d_gates) == k)
        P = C.c_void_p * max(k, 1)
        gates = None if d_gates is None else P(*[_ptr(g).value for g in d_gates])
        _check(self.lib.svo_pyramid_build_many(self._h, k, P(*[p._h.value for p in pyrs]),
                                               P(*[_ptr(i).value for i in d_images]), gates))

    def grid_keypoints(self, rows: int, cols: int, step: int) -> np.ndarray:
        cnt = C.c_int()
        _check(self.lib.svo_grid_keypoints(self._h, rows, cols, step, None, 0, MEM_HOST, C.byref(cnt)))
        out = np.empty((cnt.value, 2), np.float32)
        _check(self.lib.svo_grid_keypoints(self._h, rows, cols, step, _ptr(out), cnt.value, MEM_HOST,
                                           C.byref(cnt)))
        return out

    def lk_track(self, prev: Pyramid, nxt: Pyramid, pts: np.ndarray):
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = pts.shape[0]
        out = np.empty_like(pts)
        status = np.empty(n, np.uint8)
        err = np.empty(n, np.float32)
        mineig = np.empty(n, np.float32)
        _check(self.lib.svo_lk_track(self._h, prev._h, nxt._h, _ptr(pts), n, _ptr(out), _ptr(status),
                                     _ptr(err), _ptr(mineig), MEM_HOST))
        return out, status, err, mineig

    def lk_track_device(self, prev: Pyramid, nxt: Pyramid, pts, n, out, status, err=None, mineig=None):
        """Device-pointer form (torch tensors or raw addresses); asynchronous on the ctx stream."""
        _check(self.lib.svo_lk_track(self._h, prev._h, nxt._h, _ptr(pts), n, _ptr(out), _ptr(status),
                                     _ptr(err), _ptr(mineig), MEM_DEVICE))

    def lk_track_jobs(self, jobs):
        """``svo_lk_track_jobs``: one launch for up to 16 ``(prev, next, pts, out, status, err, mineig, gate)`` tuples of
        device tensors (err, mineig, gate may be None); asynchronous on the ctx stream."""
        k = len(jobs)
        P = C.c_void_p * k

        def col(i):
            return P(*[(j[i]._h if i < 2 else _ptr(j[i])).value for j in jobs])

        n = (C.c_int * k)(*[int(j[2].shape[0]) for j in jobs])
        _check(self.lib.svo_lk_track_jobs(self._h, k, col(0), col(1), col(2), n, col(3), col(4), col(5), col(6), col(7)))

# ---- phase-2 entry points: compaction, F-RANSAC, triangulation (host-array forms) ----------
def _ctx_method(fn):
    setattr(Context, fn.__name__, fn)
    return fn


@_ctx_method
def compact(self, mask, *arrays):
    """Order-preserving compaction of up to three float arrays by a byte mask."""
    mask = np.ascontiguousarray(mask, np.uint8)
    n = mask.shape[0]
    arrs = []
    for a in arrays:
        a = np.ascontiguousarray(a, np.float32)
        arrs.append(a.reshape(n, -1) if a.size else a.reshape(0, a.shape[1] if a.ndim > 1 else 1))
    assert 1 <= len(arrs) <= 3
    outs = [np.empty_like(a) for a in arrs]
    args = []
    for k in range(3):
        if k < len(arrs):
            args += [_ptr(arrs[k]), arrs[k].shape[1], _ptr(outs[k])]
        else:
            args += [None, 0, None]
    cnt = C.c_int()
    _check(self.lib.svo_compact(self._h, _ptr(mask), n, *args, C.byref(cnt), MEM_HOST))
    return [o[:cnt.value] for o in outs]


@_ctx_method
def fransac(self, p1, p2, threshold, confidence=0.99, max_iters=1000, seed=0):
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
    n = p1.shape[0]
    mask = np.zeros(n, np.uint8)
    F = np.zeros(9)
    cnt, iters = C.c_int(), C.c_int()
    _check(self.lib.svo_fransac(self._h, _ptr(p1), _ptr(p2), n, C.c_double(threshold), C.c_double(confidence),
                                max_iters, C.c_uint64(seed), _ptr(mask), _ptr(F), C.byref(cnt), C.byref(iters),
                                MEM_HOST))
    return cnt.value, mask, F.reshape(3, 3), iters.value


class FransacProblem(C.Structure):
    """``svo_fransac_problem``: one problem of ``svo_fransac_batch``; every pointer is a device address."""
    _fields_ = [("p1", C.c_void_p), ("p2", C.c_void_p), ("cap", C.c_int), ("d_n", C.c_void_p),
                ("threshold", C.c_double), ("confidence", C.c_double), ("max_iters", C.c_int), ("seed", C.c_uint64),
                ("mask", C.c_void_p), ("F9", C.c_void_p), ("inlier_count", C.c_void_p), ("iters_run", C.c_void_p),
                ("payload_in", C.c_void_p * 3), ("payload_out", C.c_void_p * 3), ("payload_stride", C.c_int * 3),
                ("payload_count", C.c_void_p), ("gate", C.c_void_p)]


@_ctx_method
def fransac_batch(self, problems):
    """``svo_fransac_batch``: up to 16 F-matrix RANSAC problems in one launch sequence, each with the compaction of up to
    three payload arrays by its fresh mask.  ``problems``: dicts of device tensors (or raw addresses) --
    ``p1, p2, cap, threshold, mask`` and optionally ``d_n, confidence, max_iters, seed, F9, inlier_count, iters_run,
    payload`` (a list of up to three ``(in, stride, out)``), ``payload_count, gate``.  Asynchronous on the ctx stream."""
    k = len(problems)
    arr = (FransacProblem * max(k, 1))()
    for q, p in zip(arr, problems):
        q.p1, q.p2, q.cap, q.d_n = _ptr(p["p1"]), _ptr(p["p2"]), int(p["cap"]), _ptr(p.get("d_n"))
        q.threshold, q.confidence = float(p["threshold"]), float(p.get("confidence", 0.99))
        q.max_iters, q.seed = int(p.get("max_iters", 1000)), int(p.get("seed", 0))
        q.mask, q.F9 = _ptr(p["mask"]), _ptr(p.get("F9"))
        q.inlier_count, q.iters_run = _ptr(p.get("inlier_count")), _ptr(p.get("iters_run"))
        payload = list(p.get("payload", ()))
        assert len(payload) <= 3
        for a, (src, stride, dst) in enumerate(payload):
            q.payload_in[a], q.payload_stride[a], q.payload_out[a] = _ptr(src), int(stride), _ptr(dst)
        q.payload_count, q.gate = _ptr(p.get("payload_count")), _ptr(p.get("gate"))
    _check(self.lib.svo_fransac_batch(self._h, k, arr))


def stereo_projections(fx, fy, cx, cy, baseline):
    P1, P2 = np.zeros((3, 4)), np.zeros((3, 4))
    _check(load().svo_stereo_projections(C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy),
                                         C.c_double(baseline), _ptr(P1), _ptr(P2)))
    return P1, P2


@_ctx_method
def triangulate(self, P1, P2, x1, x2):
    x1 = np.ascontiguousarray(x1, np.float32).reshape(-1, 2)
    x2 = np.ascontiguousarray(x2, np.float32).reshape(-1, 2)
    n = x1.shape[0]
    xyz = np.empty((n, 3), np.float32)
    h = np.empty((n, 4), np.float32)
    _check(self.lib.svo_triangulate(self._h, _ptr(np.ascontiguousarray(P1, np.float64)),
                                    _ptr(np.ascontiguousarray(P2, np.float64)), _ptr(x1), _ptr(x2), n,
                                    _ptr(xyz), _ptr(h), MEM_HOST))
    return xyz, h


@_ctx_method
def transform_points(self, Rt, xyz):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = np.empty_like(xyz)
    _check(self.lib.svo_transform_points(self._h, _ptr(np.ascontiguousarray(Rt, np.float64)), _ptr(xyz),
                                         xyz.shape[0], _ptr(out), MEM_HOST))
    return out


@_ctx_method
def get_colors(self, pyr, xy):
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out = np.empty((xy.shape[0], 3), np.float32)
    _check(self.lib.svo_get_colors(self._h, pyr._h, _ptr(xy), xy.shape[0], _ptr(out), MEM_HOST))
    return out


# ---- duplicate-aware replenishment: removeDuplicate / the top-up of trackSequence (src/ROSslam.py:156-169, 262-271) ----
DEDUP_BOX, DEDUP_DISC = 0, 1


@_ctx_method
def dedup_points(self, ref_xy, new_xy, radius, mode=DEDUP_BOX, ref_idx=None, wait=True):
    """``svo_dedup_points``: keep [n_new] uint8, 1 where a new point has no reference point near it (BOX: the prototype's strict
    box with its x == 0 artefact; DISC: the C++ side's norm(ref - new) < radius).  ref_idx: the reference points that take part
    (any order, repeats allowed, entries outside the array are skipped; an empty list means none), None for all.  numpy arrays, or
    device tensors, which give a device tensor back (wait=False: without waiting for the context's stream; the caller orders
    its reads after it)."""
    if _is_device(new_xy):
        import torch

        ref = ref_xy.to(torch.float32).reshape(-1, 2).contiguous()
        new = new_xy.to(torch.float32).reshape(-1, 2).contiguous()
        idx = None if ref_idx is None else torch.as_tensor(ref_idx, dtype=torch.int32, device=new.device).reshape(-1).contiguous()
        keep = torch.zeros(max(len(new), 1), dtype=torch.uint8, device=new.device)
        dummy = torch.zeros(1, dtype=torch.int32, device=new.device)      # an empty list is still a list: a non-null pointer
        torch.cuda.synchronize(new.device)
        _check(self.lib.svo_dedup_points(self._h, _ptr(ref), len(ref), _ptr(dummy if idx is not None and len(idx) == 0 else idx),
                                         0 if idx is None else len(idx), _ptr(new), len(new), C.c_double(radius), int(mode),
                                         _ptr(keep), None, MEM_DEVICE))
        if wait:
            _check(self.lib.svo_ctx_sync(self._h))
        return keep[:len(new)]
    ref = np.ascontiguousarray(ref_xy, np.float32).reshape(-1, 2)
    new = np.ascontiguousarray(new_xy, np.float32).reshape(-1, 2)
    idx = None if ref_idx is None else np.ascontiguousarray(ref_idx, np.int32).reshape(-1)
    keep = np.zeros(len(new), np.uint8)
    cnt = C.c_int()
    p_idx = None if idx is None else (C.c_int * max(len(idx), 1))(*idx.tolist())    # never null, also when the list is empty
    _check(self.lib.svo_dedup_points(self._h, _ptr(ref), len(ref), p_idx, 0 if idx is None else len(idx), _ptr(new), len(new),
                                     C.c_double(radius), int(mode), _ptr(keep), C.byref(cnt), MEM_HOST))
    assert cnt.value == int(keep.sum())
    return keep


@_ctx_method
def replenish(self, ref_xy, ref_xyz, new_xy, new_xyz, radius, Rt, mode=DEDUP_BOX, n_ref=None, counts=None, wait=True):
    """``svo_replenish``: the new points that duplicate no held point, moved with ``Rt`` (3 x 4) and in front of the camera, appended
    to the held set.  Host form (numpy arrays): -> (xy [n_out, 2], xyz [n_out, 3], n_dup, n_behind), new arrays.  Device form
    (tensors): ref_xy / ref_xyz are [cap, 2] / [cap, 3] tensors whose first ``n_ref`` rows are held; the rows behind them are
    written in place, ``counts`` (optional int32 tensor of 3: n_out, n_dup, n_behind) is filled on the device; wait=False: the call returns
    without waiting for the context's stream, as the C entry point does."""
    Rt = np.ascontiguousarray(np.asarray(Rt, np.float64).reshape(3, 4))
    if _is_device(ref_xy):
        import torch

        assert ref_xy.dtype == torch.float32 and ref_xyz.dtype == torch.float32 and ref_xy.is_contiguous() and ref_xyz.is_contiguous()
        assert n_ref is not None and ref_xy.shape[0] == ref_xyz.shape[0]
        new = new_xy.to(torch.float32).reshape(-1, 2).contiguous()
        new3 = new_xyz.to(torch.float32).reshape(-1, 3).contiguous()
        assert len(new) == len(new3)
        base = counts.data_ptr() if counts is not None else 0
        torch.cuda.synchronize(new.device)
        _check(self.lib.svo_replenish(self._h, _ptr(ref_xy), _ptr(ref_xyz), int(n_ref), int(ref_xy.shape[0]), _ptr(new), _ptr(new3),
                                      len(new), C.c_double(radius), int(mode), _ptr(Rt), C.c_void_p(base),
                                      C.c_void_p(base + 4 if base else 0), C.c_void_p(base + 8 if base else 0), MEM_DEVICE))
        if wait:
            _check(self.lib.svo_ctx_sync(self._h))
        return ref_xy, ref_xyz
    ref = np.ascontiguousarray(ref_xy, np.float32).reshape(-1, 2)
    ref3 = np.ascontiguousarray(ref_xyz, np.float32).reshape(-1, 3)
    new = np.ascontiguousarray(new_xy, np.float32).reshape(-1, 2)
    new3 = np.ascontiguousarray(new_xyz, np.float32).reshape(-1, 3)
    assert len(ref) == len(ref3) and len(new) == len(new3)
    n, cap = len(ref), len(ref) + len(new)
    xy, xyz = np.zeros((max(cap, 1), 2), np.float32), np.zeros((max(cap, 1), 3), np.float32)
    xy[:n], xyz[:n] = ref, ref3
    n_out, n_dup, n_behind = C.c_int(), C.c_int(), C.c_int()
    _check(self.lib.svo_replenish(self._h, _ptr(xy), _ptr(xyz), n, cap, _ptr(new), _ptr(new3), len(new), C.c_double(radius), int(mode),
                                  _ptr(Rt), C.byref(n_out), C.byref(n_dup), C.byref(n_behind), MEM_HOST))
    return xy[:n_out.value].copy(), xyz[:n_out.value].copy(), n_dup.value, n_behind.value


@_ctx_method
def anms(self, xy, response, num_to_keep):
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    response = np.ascontiguousarray(response, np.float32)
    n = xy.shape[0]
    idx = np.zeros(max(n, 1), np.int32)
    cnt = C.c_int()
    _check(self.lib.svo_anms(self._h, _ptr(xy), _ptr(response), n, num_to_keep, _ptr(idx), C.byref(cnt), MEM_HOST))
    return idx[:cnt.value].copy()


@_ctx_method
def orb_extract(self, img, n_features=500, fast_threshold=20):
    """cv::ORB stand-in of the loop detector (src/optimizationStuff.cpp:49-56) ->
    (xy [n,2], octave [n], response [n], dir [n,2], desc [n,8] uint32)."""
    n = C.c_int()
    if not isinstance(img, np.ndarray):      # a device tensor (H, W[, C]) uint8: the outputs come back through device buffers
        import torch

        w, h, c = _image_shape(img)
        dev = img.device
        t_xy = torch.zeros((n_features, 2), dtype=torch.float32, device=dev)
        t_oct = torch.zeros(n_features, dtype=torch.int32, device=dev)
        t_resp = torch.zeros(n_features, dtype=torch.float32, device=dev)
        t_d = torch.zeros((n_features, 2), dtype=torch.float32, device=dev)
        t_desc = torch.zeros((n_features, 8), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        _check(self.lib.svo_orb_extract(self._h, _ptr(img), w, h, c, n_features, fast_threshold, _ptr(t_xy), _ptr(t_oct),
                                        _ptr(t_resp), _ptr(t_d), _ptr(t_desc), C.byref(n), MEM_DEVICE))
        self.sync()
        k = n.value
        return (t_xy[:k].cpu().numpy(), t_oct[:k].cpu().numpy(), t_resp[:k].cpu().numpy(), t_d[:k].cpu().numpy(),
                t_desc[:k].cpu().numpy().view(np.uint32))
    img = np.ascontiguousarray(img, np.uint8)
    w, h, c = _image_shape(img)
    xy, octv = np.zeros((n_features, 2), np.float32), np.zeros(n_features, np.int32)
    resp, d = np.zeros(n_features, np.float32), np.zeros((n_features, 2), np.float32)
    desc = np.zeros((n_features, 8), np.uint32)
    _check(self.lib.svo_orb_extract(self._h, _ptr(img), w, h, c, n_features, fast_threshold, _ptr(xy), _ptr(octv),
                                    _ptr(resp), _ptr(d), _ptr(desc), C.byref(n), MEM_HOST))
    k = n.value
    return xy[:k].copy(), octv[:k].copy(), resp[:k].copy(), d[:k].copy(), desc[:k].copy()


class OrbParams(C.Structure):
    """``svo_orb_params``: shape 1 = cv::ORB's own (8 levels x 1.2, upstream's quota and pipeline), 0 = three factor-2 octaves."""
    _fields_ = [("n_features", C.c_int), ("fast_threshold", C.c_int), ("shape", C.c_int), ("n_levels", C.c_int),
                ("scale_factor", C.c_float)]


ORB_SHAPE_OCTAVES3, ORB_SHAPE_CV = 0, 1


def orb_params(**overrides) -> OrbParams:
    return _make_params(OrbParams, "svo_orb_default_params", overrides)


@_ctx_method
def orb_set_pattern(self, pattern=None):
    """``svo_orb_set_pattern``: the 256 x 4 sampling pattern (int8; cv::ORB's bit_pattern_31_ where a host has it); None =
    the seeded default."""
    if pattern is None:
        _check(self.lib.svo_orb_set_pattern(self._h, None))
        return
    pat = np.ascontiguousarray(pattern, np.int8).reshape(256, 4)
    _check(self.lib.svo_orb_set_pattern(self._h, _ptr(pat)))


@_ctx_method
def orb_extract_batch_padded(self, images, out=None, **params):
    """``svo_orb_extract_batch``: N images of one size in one set of launches.  images: list of host arrays or of device
    tensors.  -> (n [N], xy [N, nf, 2], octave [N, nf], response [N, nf], dir [N, nf, 2], desc [N, nf, 8] uint32): host
    arrays padded to the feature budget nf, image i holds n[i] features (rows beyond are zero).  Device images: the five
    outputs are sections of ONE device buffer that comes down in one copy, through a pinned buffer the context keeps.
    ``out`` = (n, xy, desc) arrays of those shapes to fill instead (-> the same three; octave / response / dir not returned)."""
    prm = orb_params(**params)
    nimg, nf = len(images), prm.n_features
    if nimg == 0:
        return (np.zeros(0, np.int32), np.zeros((0, nf, 2), np.float32), np.zeros((0, nf), np.int32), np.zeros((0, nf), np.float32),
                np.zeros((0, nf, 2), np.float32), np.zeros((0, nf, 8), np.uint32))
    first = images[0]
    w, h, c = _image_shape(first)
    n = (C.c_int * nimg)()
    e = nimg * nf
    if not isinstance(first, np.ndarray):
        import torch

        dev = first.device
        ptrs = (C.c_void_p * nimg)(*[_ptr(im).value for im in images])
        buf = torch.zeros(e * 56, dtype=torch.uint8, device=dev)   # xy 8 | octave 4 | response 4 | dir 8 | desc 32 bytes per entry
        torch.cuda.synchronize(dev)
        base = buf.data_ptr()
        _check(self.lib.svo_orb_extract_batch(self._h, ptrs, nimg, w, h, c, C.byref(prm), C.c_void_p(base), C.c_void_p(base + 8 * e),
                                              C.c_void_p(base + 12 * e), C.c_void_p(base + 16 * e), C.c_void_p(base + 24 * e), n,
                                              MEM_DEVICE))
        stage = getattr(self, "_orb_stage", None)
        if stage is None or stage.numel() < e * 56:
            stage = self._orb_stage = torch.empty(e * 56, dtype=torch.uint8).pin_memory()
        stage[:e * 56].copy_(buf)
        hb = stage[:e * 56].numpy()
        if out is not None:
            out[0][:] = n[:]
            np.copyto(out[1], hb[:8 * e].view(np.float32).reshape(nimg, nf, 2))
            np.copyto(out[2], hb[24 * e:].view(np.uint32).reshape(nimg, nf, 8))
            return out
        hb = hb.copy()     # the pinned buffer is reused by the next call
        xy = hb[:8 * e].view(np.float32).reshape(nimg, nf, 2)
        octv = hb[8 * e:12 * e].view(np.int32).reshape(nimg, nf)
        resp = hb[12 * e:16 * e].view(np.float32).reshape(nimg, nf)
        d = hb[16 * e:24 * e].view(np.float32).reshape(nimg, nf, 2)
        desc = hb[24 * e:].view(np.uint32).reshape(nimg, nf, 8)
    else:
        images = [np.ascontiguousarray(im, np.uint8) for im in images]
        ptrs = (C.c_void_p * nimg)(*[_ptr(im).value for im in images])
        xy, octv = np.zeros((nimg, nf, 2), np.float32), np.zeros((nimg, nf), np.int32)
        resp, d = np.zeros((nimg, nf), np.float32), np.zeros((nimg, nf, 2), np.float32)
        desc = np.zeros((nimg, nf, 8), np.uint32)
        _check(self.lib.svo_orb_extract_batch(self._h, ptrs, nimg, w, h, c, C.byref(prm), _ptr(xy), _ptr(octv), _ptr(resp),
                                              _ptr(d), _ptr(desc), n, MEM_HOST))
        if out is not None:
            out[0][:] = n[:]
            np.copyto(out[1], xy)
            np.copyto(out[2], desc)
            return out
    return np.array(n[:], np.int32), xy, octv, resp, d, desc


@_ctx_method
def orb_extract_batch(self, images, **params):
    """``orb_extract_batch_padded`` cut to each image's count: -> list of (xy [n,2], octave [n], response [n], dir [n,2],
    desc [n,8] uint32) per image (host arrays)."""
    n, xy, octv, resp, d, desc = self.orb_extract_batch_padded(images, **params)
    return [(xy[i, :n[i]].copy(), octv[i, :n[i]].copy(), resp[i, :n[i]].copy(), d[i, :n[i]].copy(), desc[i, :n[i]].copy())
            for i in range(len(images))]


class SgbmParams(C.Structure):
    """``svo_sgbm_params``: cv::StereoSGBM::create's arguments (defaults: the reference's, src/StereoCV.cpp:40-51)."""
    _fields_ = [(n, C.c_int) for n in ("min_disparity", "num_disparities", "block_size", "p1", "p2", "disp12_max_diff",
                                       "pre_filter_cap", "uniqueness_ratio", "speckle_window_size", "speckle_range", "mode")]


SGBM_MODE_SGBM = 0


def sgbm_params(**overrides) -> SgbmParams:
    return _make_params(SgbmParams, "svo_sgbm_default_params", overrides)


def stereo_rectify_q(fx, fy, cx, cy, tx, w, h) -> np.ndarray:
    """``svo_stereo_rectify_q``: Q of stereoRectify(K, 0, K, 0, (w, h), I, (tx, 0, 0)) as a 4 x 4 array."""
    Q = np.zeros(16, np.float64)
    _check(load().svo_stereo_rectify_q(C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), C.c_double(tx),
                                       int(w), int(h), _ptr(Q)))
    return Q.reshape(4, 4)


@_ctx_method
def sgbm(self, left, right, **params):
    """``svo_sgbm_compute`` (StereoProcess::stereoMatch, src/StereoCV.cpp:21-59): one pair (h x w or h x w x c) or a
    batch (n x h x w x c), numpy arrays or device tensors (both sides alike) -> int16 disparities x 16 of the same
    leading shape, a numpy array for host inputs and a device tensor for device inputs."""
    prm = sgbm_params(**params)
    dev = _is_device(left)
    assert dev == _is_device(right), "left and right must live in the same memory"
    shape = tuple(left.shape)
    assert tuple(right.shape) == shape
    single = len(shape) in (2, 3)   # a batch is always n x h x w x c
    if len(shape) == 2:
        n, h, w, c = 1, shape[0], shape[1], 1
    elif len(shape) == 3:
        n, (h, w, c) = 1, shape
    else:
        n, h, w, c = shape
        single = False
    if dev:
        import torch

        lt, rt = left.contiguous(), right.contiguous()
        out = torch.empty((n, h, w), dtype=torch.int16, device=left.device)
        torch.cuda.synchronize(left.device)
        _check(self.lib.svo_sgbm_compute(self._h, C.byref(prm), _ptr(lt), _ptr(rt), w, h, c, n, _ptr(out), MEM_DEVICE))
        _check(self.lib.svo_ctx_sync(self._h))
        return out[0] if single else out
    lt = np.ascontiguousarray(left, np.uint8)
    rt = np.ascontiguousarray(right, np.uint8)
    out = np.empty((n, h, w), np.int16)
    _check(self.lib.svo_sgbm_compute(self._h, C.byref(prm), _ptr(lt), _ptr(rt), w, h, c, n, _ptr(out), MEM_HOST))
    return out[0] if single else out


@_ctx_method
def stereo_reproject(self, disp, image, Q, disp_scale=1.0, z_min=0.01, z_max=5.0, flip_y=True):
    """``svo_stereo_reproject`` (StereoProcess::reprojectDisparity, src/StereoCV.cpp:227-250) -> (xyz [n,3], bgr [n,3])
    float32 host arrays, row-major order.  disp: h x w int16; image: h x w (x c) uint8 or None."""
    disp = np.ascontiguousarray(disp, np.int16)
    h, w = disp.shape
    img, c = None, 1
    if image is not None:
        img = np.ascontiguousarray(image, np.uint8)
        c = 1 if img.ndim == 2 else img.shape[2]
    q = np.ascontiguousarray(Q, np.float64).reshape(16)
    xyz = np.empty((h * w, 3), np.float32)
    bgr = np.empty((h * w, 3), np.float32) if img is not None else None
    n = C.c_int()
    _check(self.lib.svo_stereo_reproject(self._h, _ptr(disp), _ptr(img), w, h, c, _ptr(q), C.c_float(disp_scale),
                                         C.c_float(z_min), C.c_float(z_max), int(bool(flip_y)), _ptr(xyz), _ptr(bgr),
                                         C.byref(n), MEM_HOST))
    k = n.value
    return xyz[:k].copy(), (bgr[:k].copy() if bgr is not None else None)


class WlsParams(C.Structure):
    """``svo_wls_params``: the DisparityWLSFilter's settings (``lambda_`` is the header's ``lambda``)."""
    _fields_ = [("lambda_", C.c_double), ("sigma_color", C.c_double), ("lrc_thresh", C.c_int),
                ("depth_discontinuity_radius", C.c_int), ("roll_off", C.c_float), ("use_confidence", C.c_int),
                ("roi_left", C.c_int), ("roi_right", C.c_int), ("roi_top", C.c_int), ("roi_bottom", C.c_int)]


def sgbm_right_params(left: SgbmParams) -> SgbmParams:
    """``svo_sgbm_right_matcher_params``: createRightMatcher(matcher)'s parameters; run as ``ctx.sgbm(right, left, ...)``."""
    r = SgbmParams()
    load().svo_sgbm_right_matcher_params(C.byref(left), C.byref(r))
    return r


def wls_params(sgbm: SgbmParams | None = None, **overrides) -> WlsParams:
    """``svo_wls_default_params`` for a left matcher (default: the reference's), then the overrides."""
    return _make_params(WlsParams, "svo_wls_default_params", overrides, C.byref(sgbm if sgbm is not None else sgbm_params()))


def _wls_prm(sgbm: SgbmParams | None, wls) -> WlsParams:
    return _as_params(WlsParams, lambda **overrides: wls_params(sgbm, **overrides), wls)


@_ctx_method
def wls_filter(self, disp_left, disp_right, guide, wls=None, sgbm=None, want_confidence=True):
    """``svo_wls_filter``: int16 maps (h x w or n x h x w) of the left and the right matcher (disp_right may be None
    without use_confidence), guide h x w (x c) or n x h x w x c uint8 -> (filtered, confidence or None), numpy arrays
    for host inputs and device tensors for device inputs.  ``wls``: a WlsParams or a dict of overrides of the defaults
    for the left matcher ``sgbm`` (a SgbmParams; default the reference's)."""
    prm = _wls_prm(sgbm, wls)
    dev = _is_device(disp_left)
    shape = tuple(disp_left.shape)
    single = len(shape) == 2
    n, h, w = (1, *shape) if single else shape
    gshape = tuple(guide.shape)
    c = 1 if len(gshape) == (2 if single else 3) else gshape[-1]
    assert gshape[:(2 if single else 3)] == shape
    if dev:
        import torch

        lt, gt = disp_left.contiguous(), guide.contiguous()
        rt = disp_right.contiguous() if disp_right is not None else None
        out = torch.empty((n, h, w), dtype=torch.int16, device=disp_left.device)
        conf = torch.empty((n, h, w), dtype=torch.float32, device=disp_left.device) if want_confidence else None
        torch.cuda.synchronize(disp_left.device)
        _check(self.lib.svo_wls_filter(self._h, C.byref(prm), _ptr(lt), _ptr(rt), _ptr(gt), w, h, c, n, _ptr(out), _ptr(conf),
                                       MEM_DEVICE))
        _check(self.lib.svo_ctx_sync(self._h))
    else:
        lt = np.ascontiguousarray(disp_left, np.int16)
        rt = np.ascontiguousarray(disp_right, np.int16) if disp_right is not None else None
        gt = np.ascontiguousarray(guide, np.uint8)
        out = np.empty((n, h, w), np.int16)
        conf = np.empty((n, h, w), np.float32) if want_confidence else None
        _check(self.lib.svo_wls_filter(self._h, C.byref(prm), _ptr(lt), _ptr(rt), _ptr(gt), w, h, c, n, _ptr(out), _ptr(conf),
                                       MEM_HOST))
    if single:
        return out[0], (conf[0] if conf is not None else None)
    return out, conf


@_ctx_method
def sgbm_wls(self, left, right, wls=None, want_maps=True, want_confidence=True, **params):
    """``svo_sgbm_wls_compute``: both matchers and the filter on one pair or a batch (shapes as ``sgbm``) -> (filtered,
    disp_left, disp_right, confidence); the last three are None when not asked for (disp_right also without
    use_confidence's right matcher unless want_maps).  ``wls``: a WlsParams or a dict of overrides of the defaults for
    these matcher parameters; ``params``: the matcher's."""
    sp = sgbm_params(**params)
    prm = _wls_prm(sp, wls)
    dev = _is_device(left)
    assert dev == _is_device(right), "left and right must live in the same memory"
    shape = tuple(left.shape)
    assert tuple(right.shape) == shape
    single = len(shape) in (2, 3)
    if len(shape) == 2:
        n, h, w, c = 1, shape[0], shape[1], 1
    elif len(shape) == 3:
        n, (h, w, c) = 1, shape
    else:
        n, h, w, c = shape
    if dev:
        import torch

        lt, rt = left.contiguous(), right.contiguous()
        mk = lambda dt: torch.empty((n, h, w), dtype=dt, device=left.device)
        i16, f32, mem = torch.int16, torch.float32, MEM_DEVICE
        torch.cuda.synchronize(left.device)
    else:
        lt, rt = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
        mk = lambda dt: np.empty((n, h, w), dt)
        i16, f32, mem = np.int16, np.float32, MEM_HOST
    out = mk(i16)
    dl, dr = (mk(i16), mk(i16)) if want_maps else (None, None)
    conf = mk(f32) if want_confidence else None
    _check(self.lib.svo_sgbm_wls_compute(self._h, C.byref(sp), C.byref(prm), _ptr(lt), _ptr(rt), w, h, c, n, _ptr(out),
                                         _ptr(dl), _ptr(dr), _ptr(conf), mem))
    if dev:
        _check(self.lib.svo_ctx_sync(self._h))
    res = (out, dl, dr, conf)
    return tuple(a[0] if single and a is not None else a for a in res)


class BmParams(C.Structure):
    """``svo_bm_params``: cv::StereoBM's parameters (defaults: ``StereoBM::create(0, 21)``)."""
    _fields_ = [(n, C.c_int) for n in ("pre_filter_type", "pre_filter_size", "pre_filter_cap", "block_size", "min_disparity",
                                       "num_disparities", "texture_threshold", "uniqueness_ratio", "speckle_window_size",
                                       "speckle_range", "disp12_max_diff")]


BM_PREFILTER_NORMALIZED_RESPONSE, BM_PREFILTER_XSOBEL = 0, 1


def bm_params(**overrides) -> BmParams:
    return _make_params(BmParams, "svo_bm_default_params", overrides)


def bm_right_params(left: BmParams) -> BmParams:
    """``svo_bm_right_matcher_params``: createRightMatcher(matcher)'s parameters; run as ``ctx.bm(right, left, ...)``."""
    r = BmParams()
    load().svo_bm_right_matcher_params(C.byref(left), C.byref(r))
    return r


def wls_params_bm(bm: BmParams | None = None, **overrides) -> WlsParams:
    """``svo_wls_default_params_bm`` for a left block matcher (default: ``bm_params()``), then the overrides."""
    return _make_params(WlsParams, "svo_wls_default_params_bm", overrides, C.byref(bm if bm is not None else bm_params()))


def _stereo_pairs(left, right):
    """The image arguments of the dense matchers: one pair (h x w or h x w x c) or a batch (n x h x w x c), numpy arrays or
    device tensors (both sides alike) -> (left, right, n, h, w, c, single, on the device, maker of an output of n x h x w)."""
    dev = _is_device(left)
    assert dev == _is_device(right), "left and right must live in the same memory"
    shape = tuple(left.shape)
    assert tuple(right.shape) == shape
    single = len(shape) in (2, 3)   # a batch is always n x h x w x c
    if len(shape) == 2:
        n, h, w, c = 1, shape[0], shape[1], 1
    elif len(shape) == 3:
        n, (h, w, c) = 1, shape
    else:
        n, h, w, c = shape
    if dev:
        import torch

        names = {np.int16: torch.int16, np.float32: torch.float32, np.uint8: torch.uint8}
        mk = lambda dt: torch.empty((n, h, w), dtype=names[dt], device=left.device)
        lt, rt = left.contiguous(), right.contiguous()
        torch.cuda.synchronize(left.device)
    else:
        mk = lambda dt: np.empty((n, h, w), dt)
        lt, rt = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
    return lt, rt, n, h, w, c, single, dev, mk


def _bm_prm(params) -> BmParams:
    prm = params.pop("params", None)
    return _as_params(BmParams, bm_params, prm) if prm is not None else bm_params(**params)


@_ctx_method
def bm(self, left, right, **params):
    """``svo_bm_compute`` (cv::StereoBM): images as ``sgbm`` takes them -> int16 disparities x 16 of the same leading shape, a
    numpy array for host inputs and a device tensor for device inputs.  ``params``: fields of ``svo_bm_params``, or
    ``params=`` a BmParams."""
    prm = _bm_prm(params)
    lt, rt, n, h, w, c, single, dev, mk = _stereo_pairs(left, right)
    out = mk(np.int16)
    _check(self.lib.svo_bm_compute(self._h, C.byref(prm), _ptr(lt), _ptr(rt), w, h, c, n, _ptr(out), _mem_of(dev)))
    if dev:
        _check(self.lib.svo_ctx_sync(self._h))
    return out[0] if single else out


@_ctx_method
def bm_wls(self, left, right, wls=None, want_maps=True, want_confidence=True, **params):
    """``svo_bm_wls_compute``: both block matchers and the filter on one pair or a batch -> (filtered, disp_left, disp_right,
    confidence) as ``sgbm_wls`` returns them.  ``wls``: a WlsParams or a dict of overrides of ``wls_params_bm`` for these
    matcher parameters."""
    bp = _bm_prm(params)
    prm = _as_params(WlsParams, lambda **overrides: wls_params_bm(bp, **overrides), wls)
    lt, rt, n, h, w, c, single, dev, mk = _stereo_pairs(left, right)
    out = mk(np.int16)
    dl, dr = (mk(np.int16), mk(np.int16)) if want_maps else (None, None)
    conf = mk(np.float32) if want_confidence else None
    _check(self.lib.svo_bm_wls_compute(self._h, C.byref(bp), C.byref(prm), _ptr(lt), _ptr(rt), w, h, c, n, _ptr(out), _ptr(dl),
                                       _ptr(dr), _ptr(conf), _mem_of(dev)))
    if dev:
        _check(self.lib.svo_ctx_sync(self._h))
    return tuple(a[0] if single and a is not None else a for a in (out, dl, dr, conf))


@_ctx_method
def bm_prefilter(self, image, cap=31):
    """``svo_bm_prefilter``: the XSOBEL pre-filter of one h x w (x c) image (numpy array or device tensor) -> uint8 h x w."""
    dev = _is_device(image)
    w, h, c = _image_shape(image)
    if dev:
        import torch

        img = image.contiguous()
        out = torch.empty((h, w), dtype=torch.uint8, device=image.device)
        torch.cuda.synchronize(image.device)
    else:
        img = np.ascontiguousarray(image, np.uint8)
        out = np.empty((h, w), np.uint8)
    _check(self.lib.svo_bm_prefilter(self._h, _ptr(img), w, h, c, int(cap), _ptr(out), _mem_of(dev)))
    if dev:
        _check(self.lib.svo_ctx_sync(self._h))
    return out


MATH_FN = {"sin": 0, "cos": 1, "acos": 2, "cbrt": 3, "log": 4, "exp": 5}
MATH_EXP = MATH_FN["exp"]


@_ctx_method
def math_eval(self, fn: str, x) -> np.ndarray:
    """include/svo_math.h evaluated on the device (svo_math_eval); the parity tests compare the bits with
    the host build of the same header."""
    x = np.ascontiguousarray(x, np.float64).ravel()
    y = np.empty_like(x)
    _check(self.lib.svo_math_eval(self._h, MATH_FN[fn], _ptr(x), x.size, _ptr(y), MEM_HOST))
    return y


SCAN_KINDS = {"256_int": (0, "int32"), "1024_uint": (1, "uint32"), "1024_u64": (2, "uint64")}


@_ctx_method
def selftest_scan(self, kind: str, d_in, n: int, d_out, d_total) -> None:
    """svo_selftest_scan: ``d_out[:n]`` = the exclusive prefix sums of ``d_in[:n]`` and ``d_total[0]`` their sum, by one
    workgroup of csrc/scan_ops.hip.h's block scan.  Device arrays of SCAN_KINDS[kind]'s element size; ``d_out`` may be
    ``d_in``."""
    _check(self.lib.svo_selftest_scan(self._h, SCAN_KINDS[kind][0], _ptr(d_in), int(n), _ptr(d_out), _ptr(d_total)))


class SiftParams(C.Structure):
    """``svo_sift_params``: cv::xfeatures2d::SIFT::create's arguments (n_features 0 = all)."""
    _fields_ = [("n_features", C.c_int), ("n_octave_layers", C.c_int), ("contrast_threshold", C.c_double),
                ("edge_threshold", C.c_double), ("sigma", C.c_double)]


def sift_params(**overrides) -> SiftParams:
    return _make_params(SiftParams, "svo_sift_default_params", overrides)


def _sift_prm(params) -> SiftParams:
    return _as_params(SiftParams, sift_params, params)


# ---- the batched detectors' shared call: svo_{sift,surf}_extract_batch, svo_fast_{detect,anms}_batch, svo_star_detect_batch ----
def _column_layout(spec, e):
    """Where the output columns of a batched detector lie on the device.  ``spec``: [(name, np.float32 or np.int32, trailing
    width)] in the order of the entry point's arguments; ``e``: entries per column (images x capacity).  The float32 columns lie
    back to back in one buffer and the int32 columns in another -> ({name: (dtype, byte offset in its buffer, width)}, bytes
    of the float buffer, bytes of the int buffer).  The pointers handed to the library and the views of what came back are both
    taken from this."""
    cols, size = {}, {np.float32: 0, np.int32: 0}
    for name, dtype, width in spec:
        cols[name] = (dtype, size[dtype], width)
        size[dtype] += 4 * e * width
    return cols, size[np.float32], size[np.int32]


def _batch_images(images):
    """images of one batch, where the first one lives -> (the images made contiguous, their pointer array, device?)"""
    dev = _is_device(images[0])
    images = [im.contiguous() for im in images] if dev else [np.ascontiguousarray(im, np.uint8) for im in images]
    return images, (C.c_void_p * max(len(images), 1))(*[_ptr(im).value for im in images]), dev


def _raise_with_counts(self, rc, n, nimg, prefix=None):
    """Raise the SvoError of ``rc`` with the per-image counts in ``needed`` (and what did fit in ``prefix``)."""
    err = SvoError(rc, self.lib.svo_last_error().decode(errors="replace"))
    err.needed = list(n[:nimg])
    if prefix is not None:
        err.prefix = prefix
    raise err


def _batch_call(self, fn, images, spec, cap, pre_args, post_args=(), accept=(SVO_OK,)):
    """``fn(ctx, image pointers, nimg, w, h, c, *pre_args, a pointer per column of spec, *post_args, counts, mem)`` on host arrays
    or device tensors.  Host: one zeroed array per column.  Device: one zeroed float32 buffer and, if ``spec`` has int32 columns,
    one int32 buffer (``_column_layout``), one ``torch.cuda.synchronize`` before the call, then ``svo_ctx_sync`` and one copy down
    per buffer.  -> ({name: host array [nimg, cap(, width)]}, counts [nimg], rc); an ``rc`` outside ``accept`` raises with the
    counts before anything is waited for."""
    nimg, e = len(images), len(images) * cap
    w, h, c = _image_shape(images[0])
    images, ptrs, dev = _batch_images(images)
    n = (C.c_int * max(nimg, 1))()
    cols, fbytes, ibytes = _column_layout(spec, e)
    shape = lambda width: (nimg, cap) + ((width,) if width > 1 else ())
    if dev:
        import torch

        bufs = {np.float32: torch.zeros(fbytes // 4, dtype=torch.float32, device=images[0].device)}
        if ibytes:
            bufs[np.int32] = torch.zeros(ibytes // 4, dtype=torch.int32, device=images[0].device)
        torch.cuda.synchronize(images[0].device)
        outs = [C.c_void_p(bufs[dtype].data_ptr() + off) for dtype, off, _ in cols.values()]
    else:
        host = {name: np.zeros(shape(width), dtype) for name, (dtype, _, width) in cols.items()}
        outs = [_ptr(a) for a in host.values()]
    rc = fn(self._h, ptrs, nimg, w, h, c, *pre_args, *outs, *post_args, n, _mem_of(dev))
    if rc not in accept:
        _raise_with_counts(self, rc, n, nimg)
    if dev:
        _check(self.lib.svo_ctx_sync(self._h))
        flat = {dtype: b.cpu().numpy().view(np.uint8) for dtype, b in bufs.items()}
        host = {name: flat[dtype][off:off + 4 * e * width].view(dtype).reshape(shape(width))
                for name, (dtype, off, width) in cols.items()}
    return host, list(n[:nimg]), rc


def _cut(columns, counts):
    """padded [nimg, cap, ...] columns (None stays None) -> per image, a tuple of copies of its first ``counts[i]`` rows"""
    return [tuple(None if a is None else a[i, :k].copy() for a in columns) for i, k in enumerate(counts)]


_SIFT_COLUMNS = [("xy", np.float32, 2), ("size", np.float32, 1), ("angle", np.float32, 1), ("response", np.float32, 1),
                 ("octave", np.int32, 1), ("desc", np.float32, 128)]


@_ctx_method
def sift_extract(self, images, params=None, cap=20000, descriptors=True):
    """``svo_sift_extract_batch``: 1 ... 16 images of one size (host arrays or device tensors) in one set of launches -> per
    image (xy [n, 2], size [n], angle [n], response [n] float32, octave [n] int32 -- cv's packed field --, desc [n, 128] float32
    or None), host arrays in the recipe's order.  More than ``cap`` key points in an image: SvoError(SVO_ERR_CAPACITY) whose
    ``needed`` lists the counts."""
    prm = _sift_prm(params)
    # without descriptors the column is not allocated and the library gets a null pointer in its place
    spec, no_desc = (_SIFT_COLUMNS, ()) if descriptors else (_SIFT_COLUMNS[:-1], (None,))
    col, n, _ = _batch_call(self, self.lib.svo_sift_extract_batch, images, spec, cap, (C.byref(prm), cap), no_desc)
    return _cut([*col.values(), *no_desc], n)


@_ctx_method
def sift_describe(self, image, xy, size, angle, octave, params=None) -> np.ndarray:
    """``svo_sift_describe``: detector->compute(image, keypoints) -> desc [n, 128] float32 (host arrays in and out)."""
    prm = _sift_prm(params)
    img = np.ascontiguousarray(image, np.uint8)
    w, h, c = _image_shape(img)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    size, angle = np.ascontiguousarray(size, np.float32), np.ascontiguousarray(angle, np.float32)
    octave = np.ascontiguousarray(octave, np.int32)
    desc = np.zeros((len(xy), 128), np.float32)
    _check(self.lib.svo_sift_describe(self._h, _ptr(img), w, h, c, C.byref(prm), _ptr(xy), _ptr(size), _ptr(angle), _ptr(octave),
                                      len(xy), _ptr(desc), MEM_HOST))
    return desc


@_ctx_method
def sift_pyramid(self, image, params=None):
    """``svo_sift_pyramid`` (diagnostics) -> (gauss, dog): per octave float32 arrays [layers + 3, h, w] / [layers + 2, h, w]."""
    prm = _sift_prm(params)
    img = np.ascontiguousarray(image, np.uint8)
    w, h, c = _image_shape(img)
    no, ow, oh = C.c_int(), (C.c_int * 16)(), (C.c_int * 16)()
    _check(self.lib.svo_sift_pyramid_layout(w, h, prm.n_octave_layers, C.byref(no), ow, oh))
    px = [ow[o] * oh[o] for o in range(no.value)]
    nl = prm.n_octave_layers
    g, d = np.zeros(sum(px) * (nl + 3), np.float32), np.zeros(sum(px) * (nl + 2), np.float32)
    _check(self.lib.svo_sift_pyramid(self._h, _ptr(img), w, h, c, C.byref(prm), _ptr(g), _ptr(d), MEM_HOST))
    gauss, dog, a, b = [], [], 0, 0
    for o in range(no.value):
        gauss.append(g[a:a + px[o] * (nl + 3)].reshape(nl + 3, oh[o], ow[o]))
        dog.append(d[b:b + px[o] * (nl + 2)].reshape(nl + 2, oh[o], ow[o]))
        a, b = a + px[o] * (nl + 3), b + px[o] * (nl + 2)
    return gauss, dog


class FastParams(C.Structure):
    """``svo_fast_params``: cv::FAST's arguments and retainBest's budget (max_keypoints 0 = all)."""
    _fields_ = [("threshold", C.c_int), ("nonmax_suppression", C.c_int), ("max_keypoints", C.c_int)]


def fast_params(**overrides) -> FastParams:
    return _make_params(FastParams, "svo_fast_default_params", overrides)


_FAST_COLUMNS = [("xy", np.float32, 2), ("response", np.float32, 1)]


def _fast_call(self, images, prm, cap, keep, score):
    """Both FAST entry points: per image (xy [n, 2], response [n][, score [h, w]]) as host arrays."""
    w, h, c = _image_shape(images[0])
    if cap is None:
        cap = max((w - 6) * (h - 6), 1)          # no image has more key points than interior pixels
    if keep is not None:
        col, n, _ = _batch_call(self, self.lib.svo_fast_anms_batch, images, _FAST_COLUMNS, cap, (C.byref(prm), keep, cap))
        return _cut(col.values(), n)
    sb = None
    if score:                                    # a [nimg, h, w] uint8 plane of its own, where the images live
        if _is_device(images[0]):
            import torch

            sb = torch.zeros((len(images), h, w), dtype=torch.uint8, device=images[0].device)
        else:
            sb = np.zeros((len(images), h, w), np.uint8)
    col, n, _ = _batch_call(self, self.lib.svo_fast_detect_batch, images, _FAST_COLUMNS, cap, (C.byref(prm), cap), (_ptr(sb),))
    if not score:
        return _cut(col.values(), n)
    sb = sb.cpu().numpy() if _is_device(sb) else sb
    return [kp + (sb[i].copy(),) for i, kp in enumerate(_cut(col.values(), n))]


@_ctx_method
def fast_detect(self, images, threshold=10, nonmax=True, max_keypoints=0, cap=None, score=False):
    """``svo_fast_detect_batch``: cv::FAST (TYPE_9_16) on 1 ... 16 images of one size (host arrays or device tensors) in one set
    of launches -> per image (xy [n, 2], response [n] float32[, score [h, w] uint8]) in row-major order.  More than ``cap`` key
    points in an image: SvoError(SVO_ERR_CAPACITY) whose ``needed`` lists the counts."""
    prm = fast_params(threshold=threshold, nonmax_suppression=int(bool(nonmax)), max_keypoints=max_keypoints)
    return _fast_call(self, images, prm, cap, None, score)


@_ctx_method
def fast_anms(self, images, num_to_keep, threshold=10, nonmax=True, max_keypoints=0, cap=None):
    """``svo_fast_anms_batch``: FAST, then adaptive non-maximal suppression of each image's key points without leaving the
    device -> per image (xy [k, 2], response [k]) in ANMS's response-sorted order."""
    prm = fast_params(threshold=threshold, nonmax_suppression=int(bool(nonmax)), max_keypoints=max_keypoints)
    return _fast_call(self, images, prm, cap, int(num_to_keep), False)


class GfttParams(C.Structure):
    """``svo_gftt_params``: goodFeaturesToTrack's arguments (max_corners <= 0 = all)."""
    _fields_ = [("max_corners", C.c_int), ("block_size", C.c_int), ("use_harris", C.c_int), ("pad", C.c_int),
                ("quality_level", C.c_double), ("min_distance", C.c_double), ("k", C.c_double)]


def gftt_params(**overrides) -> GfttParams:
    return _make_params(GfttParams, "svo_gftt_default_params", overrides)


_GFTT_COLUMNS = [("xy", np.float32, 2), ("response", np.float32, 1)]


@_ctx_method
def gftt_detect(self, images, masks=None, params=None, cap=None, **overrides):
    """``svo_gftt_detect_batch``: cv::goodFeaturesToTrack on 1 ... 16 images of one size (host arrays or device tensors) in one set
    of launches -> per image (xy [n, 2], response [n]) float32 host arrays in acceptance order.  ``masks``: None, or one entry per
    image, each None or an [h, w] uint8 array / tensor where the images live.  ``params``: a GfttParams or a dict; keyword
    arguments override its fields.  More than ``cap`` corners in an image: SvoError(SVO_ERR_CAPACITY) whose ``needed`` lists the
    counts."""
    prm = _as_params(GfttParams, gftt_params, params)
    for k, v in overrides.items():
        assert hasattr(prm, k), k
        setattr(prm, k, v)
    w, h, c = _image_shape(images[0])
    if cap is None:
        cap = max((w - 2) * (h - 2), 1)          # no image has more corners than interior pixels
    mptrs = None
    if masks is not None:
        assert len(masks) == len(images)
        dev = _is_device(images[0])
        masks = [None if m is None else m.contiguous() if dev else np.ascontiguousarray(m, np.uint8) for m in masks]
        mptrs = (C.c_void_p * max(len(masks), 1))(*[_ptr(m).value for m in masks])
    fn = lambda ctx, ptrs, *rest: self.lib.svo_gftt_detect_batch(ctx, ptrs, mptrs, *rest)   # the masks follow the images
    col, n, _ = _batch_call(self, fn, images, _GFTT_COLUMNS, cap, (C.byref(prm), cap))
    return _cut(col.values(), n)


@_ctx_method
def gftt_response(self, image, params=None, **overrides) -> np.ndarray:
    """``svo_gftt_response`` -> the corner measure of every pixel before thresholding, [h, w] float32 (host array or device
    tensor in, host array out)."""
    prm = _as_params(GfttParams, gftt_params, params)
    for k, v in overrides.items():
        assert hasattr(prm, k), k
        setattr(prm, k, v)
    w, h, c = _image_shape(image)
    dev = _is_device(image)
    if dev:
        import torch

        image = image.contiguous()
        eig = torch.zeros((h, w), dtype=torch.float32, device=image.device)
        torch.cuda.synchronize(image.device)
    else:
        image, eig = np.ascontiguousarray(image, np.uint8), np.zeros((h, w), np.float32)
    _check(self.lib.svo_gftt_response(self._h, _ptr(image), w, h, c, C.byref(prm), _ptr(eig), _mem_of(dev)))
    if dev:
        _check(self.lib.svo_ctx_sync(self._h))
        eig = eig.cpu().numpy()
    return eig


class StarParams(C.Structure):
    """``svo_star_params``: xfeatures2d::StarDetector::create's arguments."""
    _fields_ = [("max_size", C.c_int), ("response_threshold", C.c_int), ("line_threshold_projected", C.c_int),
                ("line_threshold_binarized", C.c_int), ("suppress_nonmax_size", C.c_int)]


def star_params(**overrides) -> StarParams:
    return _make_params(StarParams, "svo_star_default_params", overrides)


def _star_prm(params) -> StarParams:
    return _as_params(StarParams, star_params, params)


def star_layout(w, h, max_size=45):
    """``svo_star_layout`` -> (npatterns, max_idx, border).  Host only."""
    out = [C.c_int() for _ in range(3)]
    _check(load().svo_star_layout(int(w), int(h), int(max_size), *[C.byref(o) for o in out]))
    return tuple(o.value for o in out)


def _star_images(images, mem):
    """The images where ``mem`` wants them (None: where they are) -> (images, is_device)."""
    dev = _is_device(images[0]) if mem is None else mem == MEM_DEVICE
    if dev:
        import torch

        images = [(im if _is_device(im) else torch.from_numpy(np.ascontiguousarray(im, np.uint8)).cuda()).contiguous() for im in images]
        torch.cuda.synchronize(images[0].device)
    else:
        images = [np.ascontiguousarray(im.cpu().numpy() if _is_device(im) else im, np.uint8) for im in images]
    return images, dev


_STAR_COLUMNS = [("xy", np.float32, 2), ("size", np.float32, 1), ("response", np.float32, 1)]


@_ctx_method
def star_detect(self, images, prm=None, cap=None, mem=None):
    """``svo_star_detect_batch``: the Star (CenSurE) detector on 1 ... 16 images of one size (host arrays or device tensors; ``mem``
    moves them first) in one set of launches -> per image (xy [n, 2], size [n], response [n]) float32 host arrays, a tile's
    maximum before its minimum, tiles in row-major order.  More than ``cap`` key points in an image:
    SvoError(SVO_ERR_CAPACITY) whose ``needed`` lists the counts."""
    prm = _star_prm(prm)
    w, h, c = _image_shape(images[0])
    if cap is None:
        cap = max(2 * w * h, 1)                  # a pixel is at most a maximum and a minimum
    images, _ = _star_images(images, mem)
    col, n, _ = _batch_call(self, self.lib.svo_star_detect_batch, images, _STAR_COLUMNS, cap, (C.byref(prm), cap))
    return _cut(col.values(), n)


@_ctx_method
def star_responses(self, image, prm=None, mem=None):
    """``svo_star_responses`` (diagnostics) -> (response [h, w] float32, size [h, w] int16, border) as host values."""
    prm = _star_prm(prm)
    w, h, c = _image_shape(image)
    (img,), dev = _star_images([image], mem)
    border = C.c_int(-1)
    if dev:
        import torch

        resp = torch.zeros((h, w), dtype=torch.float32, device=img.device)
        size = torch.zeros((h, w), dtype=torch.int16, device=img.device)
        torch.cuda.synchronize(img.device)
    else:
        resp, size = np.zeros((h, w), np.float32), np.zeros((h, w), np.int16)
    _check(self.lib.svo_star_responses(self._h, _ptr(img), w, h, c, C.byref(prm), _ptr(resp), _ptr(size), C.byref(border),
                                       _mem_of(dev)))
    if dev:
        _check(self.lib.svo_ctx_sync(self._h))
        resp, size = resp.cpu().numpy(), size.cpu().numpy()
    return resp, size, border.value


def brief_default_pattern(bytes=32) -> np.ndarray:
    """``svo_brief_default_pattern``: the library's own test table of a descriptor length, [8 * bytes, 4] int8 rows of
    (y1, x1, y2, x2).  Host only."""
    pat = np.zeros((8 * max(int(bytes), 0), 4), np.int8)
    _check(load().svo_brief_default_pattern(int(bytes), _ptr(pat) if pat.size else None))
    return pat


@_ctx_method
def brief_set_pattern(self, pattern=None, bytes=32):
    """``svo_brief_set_pattern``: the test table of one descriptor length (cv's generated_NN.i where a host has it); None = the
    default."""
    if pattern is None:
        _check(self.lib.svo_brief_set_pattern(self._h, int(bytes), None))
        return
    pat = np.ascontiguousarray(pattern, np.int8).reshape(8 * int(bytes), 4)
    _check(self.lib.svo_brief_set_pattern(self._h, int(bytes), _ptr(pat)))


@_ctx_method
def brief_describe(self, images, xy_list, bytes=32):
    """``svo_brief_describe_batch``: 1 ... 16 images of one size and the key points of each ([n, 2] float32; host arrays, or device
    tensors when the images are) in one set of launches -> per image (desc [m, bytes] uint8, kept_index [m] int32), host arrays:
    the descriptors of the key points runByImageBorder keeps and their indices into the image's list, in order."""
    nimg = len(images)
    assert nimg == len(xy_list)
    w, h, c = _image_shape(images[0])
    n_in = (C.c_int * max(nimg, 1))(*[int(len(xy)) for xy in xy_list])
    n_out = (C.c_int * max(nimg, 1))()
    cap = max([1] + [int(len(xy)) for xy in xy_list])
    nb = int(bytes)
    images, ptrs, dev = _batch_images(images)
    if dev:
        import torch

        device = images[0].device
        xy = torch.zeros((nimg, cap, 2), dtype=torch.float32, device=device)
        for i, p in enumerate(xy_list):
            if len(p):
                xy[i, :len(p)] = torch.as_tensor(p, dtype=torch.float32, device=device).reshape(-1, 2)
        kept = torch.zeros((nimg, cap), dtype=torch.int32, device=device)
        desc = torch.zeros((nimg, cap, max(nb, 1)), dtype=torch.uint8, device=device)
        torch.cuda.synchronize(device)
    else:
        xy = np.zeros((nimg, cap, 2), np.float32)
        for i, p in enumerate(xy_list):
            if len(p):
                xy[i, :len(p)] = np.asarray(p, np.float32).reshape(-1, 2)
        kept, desc = np.zeros((nimg, cap), np.int32), np.zeros((nimg, cap, max(nb, 1)), np.uint8)
    _check(self.lib.svo_brief_describe_batch(self._h, ptrs, nimg, w, h, c, nb, _ptr(xy), n_in, cap, _ptr(kept), _ptr(desc), n_out,
                                             _mem_of(dev)))
    if dev:
        _check(self.lib.svo_ctx_sync(self._h))
        kept, desc = kept.cpu().numpy(), desc.cpu().numpy()
    return _cut((desc, kept), n_out[:nimg])


@_ctx_method
def brief_integral(self, image) -> np.ndarray:
    """``svo_brief_integral`` (diagnostics) -> the [h + 1, w + 1] int32 integral image of the grey image (host arrays)."""
    img = np.ascontiguousarray(image, np.uint8)
    w, h, c = _image_shape(img)
    out = np.zeros((h + 1, w + 1), np.int32)
    _check(self.lib.svo_brief_integral(self._h, _ptr(img), w, h, c, _ptr(out), MEM_HOST))
    return out


class SurfParams(C.Structure):
    """``svo_surf_params``: cv::xfeatures2d::SURF::create's arguments (extended must stay 0)."""
    _fields_ = [("hessian_threshold", C.c_double), ("n_octaves", C.c_int), ("n_octave_layers", C.c_int), ("extended", C.c_int),
                ("upright", C.c_int)]


def surf_params(**overrides) -> SurfParams:
    return _make_params(SurfParams, "svo_surf_default_params", overrides)


def _surf_prm(params) -> SurfParams:
    return _as_params(SurfParams, surf_params, params)


_SURF_COLUMNS = [("xy", np.float32, 2), ("size", np.float32, 1), ("angle", np.float32, 1), ("response", np.float32, 1),
                 ("octave", np.int32, 1), ("laplacian", np.int32, 1), ("desc", np.float32, 64)]


@_ctx_method
def surf_extract(self, images, params=None, cap=20000, descriptors=True):
    """``svo_surf_extract_batch``: 1 ... 16 images of one size (host arrays or device tensors) in one set of launches -> per
    image (xy [n, 2], size [n], angle [n], response [n] float32, octave [n], laplacian [n] int32, desc [n, 64] float32 or
    None), host arrays in the recipe's order.  More than ``cap`` key points in an image: SvoError(SVO_ERR_CAPACITY) whose
    ``needed`` lists the counts and whose ``prefix`` holds the first ``cap`` key points of every image."""
    prm = _surf_prm(params)
    # without descriptors the column is not allocated and the library gets a null pointer in its place
    spec, no_desc = (_SURF_COLUMNS, ()) if descriptors else (_SURF_COLUMNS[:-1], (None,))
    col, n, rc = _batch_call(self, self.lib.svo_surf_extract_batch, images, spec, cap, (C.byref(prm), cap), no_desc,
                             accept=(SVO_OK, SVO_ERR_CAPACITY))
    out = _cut([*col.values(), *no_desc], [min(k, cap) for k in n])      # over capacity: the first ``cap`` key points were written
    if rc != SVO_OK:
        _raise_with_counts(self, rc, n, len(images), prefix=out)
    return out


@_ctx_method
def surf_describe(self, image, xy, size, params=None):
    """``svo_surf_describe``: detector->compute(image, keypoints) -> (angle [n] float32, desc [n, 64] float32, kept [n] uint8);
    host arrays in and out."""
    prm = _surf_prm(params)
    img = np.ascontiguousarray(image, np.uint8)
    w, h, c = _image_shape(img)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    size = np.ascontiguousarray(size, np.float32).reshape(-1)
    assert len(size) == len(xy)
    angle, desc, kept = np.zeros(len(xy), np.float32), np.zeros((len(xy), 64), np.float32), np.zeros(len(xy), np.uint8)
    _check(self.lib.svo_surf_describe(self._h, _ptr(img), w, h, c, C.byref(prm), _ptr(xy), _ptr(size), len(xy), _ptr(angle),
                                      _ptr(desc), _ptr(kept), MEM_HOST))
    return angle, desc, kept


def surf_layers_layout(w, h, n_octaves=4, n_octave_layers=3):
    """``svo_surf_layers_layout`` -> (sizes, steps, lw, lh), one int per layer, octave after octave.  Host only."""
    m = max(n_octaves * (n_octave_layers + 2), 1)
    arr = [(C.c_int * m)() for _ in range(4)]
    _check(load().svo_surf_layers_layout(w, h, n_octaves, n_octave_layers, *arr))
    return tuple(list(a) for a in arr)


@_ctx_method
def surf_layers(self, image, params=None):
    """``svo_surf_layers`` (diagnostics) -> (det, trace): one float32 plane per layer, octave after octave."""
    prm = _surf_prm(params)
    img = np.ascontiguousarray(image, np.uint8)
    w, h, c = _image_shape(img)
    _, _, lw, lh = surf_layers_layout(w, h, prm.n_octaves, prm.n_octave_layers)
    total = sum(a * b for a, b in zip(lw, lh))
    d, t = np.zeros(max(total, 1), np.float32), np.zeros(max(total, 1), np.float32)
    _check(self.lib.svo_surf_layers(self._h, _ptr(img), w, h, c, C.byref(prm), _ptr(d), _ptr(t), MEM_HOST))
    det, trace, a = [], [], 0
    for pw, ph in zip(lw, lh):
        det.append(d[a:a + pw * ph].reshape(ph, pw))
        trace.append(t[a:a + pw * ph].reshape(ph, pw))
        a += pw * ph
    return det, trace


@_ctx_method
def sor_filter(self, xyz, color=None, mean_k=200, stddev_mul=0.01, z_limit=500.0):
    """visualSLAM::SORcloud (src/rosFuncs.cpp:9-39) -> (xyz_kept, color_kept or None, mean_dist)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    col = None if color is None else np.ascontiguousarray(color, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    xo, co, md = np.zeros((max(n, 1), 3), np.float32), np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.float32)
    kept, passed = C.c_int(), C.c_int()
    _check(self.lib.svo_sor_filter(self._h, _ptr(xyz), _ptr(col), n, int(mean_k), C.c_double(stddev_mul),
                                   C.c_float(z_limit), _ptr(xo), _ptr(co) if col is not None else _ptr(None),
                                   C.byref(kept), _ptr(md), C.byref(passed), MEM_HOST))
    return xo[:kept.value].copy(), (co[:kept.value].copy() if col is not None else None), md[:passed.value].copy()


@_ctx_method
def sor_filter_large(self, xyz, color=None, mean_k=20, stddev_mul=0.8, z_limit=0.0):
    """``svo_sor_filter_large``: sor_filter's algorithm and results for up to 2^22 points; the defaults are
    StereoProcess::pclPublish's (src/StereoCV.cpp:289-293).  numpy arrays, or device tensors (float32, n x 3, on the
    context's device) which give device tensors back -> (xyz_kept, color_kept or None, mean_dist)."""
    if _is_device(xyz):
        import torch

        assert color is None or _is_device(color), "xyz and color must live in the same memory"
        xt = xyz.reshape(-1, 3).contiguous()
        ct = None if color is None else color.reshape(-1, 3).contiguous()
        assert xt.dtype == torch.float32 and (ct is None or (ct.dtype == torch.float32 and ct.shape == xt.shape))
        n = xt.shape[0]
        xo = torch.empty((max(n, 1), 3), dtype=torch.float32, device=xt.device)
        co = torch.empty_like(xo) if ct is not None else None
        md = torch.empty(max(n, 1), dtype=torch.float32, device=xt.device)
        torch.cuda.synchronize(xt.device)
        mem = MEM_DEVICE
    else:
        xt = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        ct = None if color is None else np.ascontiguousarray(color, np.float32).reshape(-1, 3)
        n = xt.shape[0]
        xo, md = np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.float32)
        co = np.zeros((max(n, 1), 3), np.float32) if ct is not None else None
        mem = MEM_HOST
    kept, passed = C.c_int(), C.c_int()
    _check(self.lib.svo_sor_filter_large(self._h, _ptr(xt), _ptr(ct), n, int(mean_k), C.c_double(stddev_mul),
                                         C.c_float(z_limit), _ptr(xo), _ptr(co), C.byref(kept), _ptr(md), C.byref(passed),
                                         mem))
    k, p = kept.value, passed.value
    if mem == MEM_DEVICE:
        return xo[:k], (co[:k] if co is not None else None), md[:p]
    return xo[:k].copy(), (co[:k].copy() if co is not None else None), md[:p].copy()


def voxel_grid(min_xyz, max_xyz, voxel_size):
    """``svo_voxel_grid`` (host code, no context): the grid of a cloud's finite bounds -> (min_bound [3] float64, cells [3]
    int64, fits); fits is False when an axis spans 2^21 cells or more, which ``voxel_downsample`` refuses."""
    lo = np.ascontiguousarray(min_xyz, np.float32).reshape(3)
    hi = np.ascontiguousarray(max_xyz, np.float32).reshape(3)
    mb, cells = np.zeros(3, np.float64), np.zeros(3, np.int64)
    rc = load().svo_voxel_grid(_ptr(lo), _ptr(hi), C.c_double(voxel_size), _ptr(mb), _ptr(cells))
    if rc != SVO_ERR_CAPACITY:
        _check(rc)
    return mb, cells, rc == SVO_OK


@_ctx_method
def voxel_downsample(self, xyz, voxel_size, color=None, trace=False, mem=None):
    """``svo_voxel_downsample``: one point per occupied voxel of edge ``voxel_size``, the mean of the voxel's points (and colours),
    in ascending voxel key order.  numpy arrays, or device tensors (float32, n x 3, on the context's device) which give device
    tensors back; ``mem`` may say which explicitly.  -> (xyz_out, color_out or None[, point_voxel, voxel_count]); point_voxel:
    the output row of every input point, -1 for a point with a non-finite coordinate."""
    device = _is_device(xyz) if mem is None else mem == MEM_DEVICE
    if device:
        import torch

        assert _is_device(xyz) and (color is None or _is_device(color)), "xyz and color must live in the same memory"
        xt = xyz.reshape(-1, 3).contiguous()
        ct = None if color is None else color.reshape(-1, 3).contiguous()
        assert xt.dtype == torch.float32 and (ct is None or (ct.dtype == torch.float32 and ct.shape == xt.shape))
        n = xt.shape[0]
        xo = torch.empty((max(n, 1), 3), dtype=torch.float32, device=xt.device)
        co = torch.empty_like(xo) if ct is not None else None
        pv = torch.empty(max(n, 1), dtype=torch.int32, device=xt.device) if trace else None
        vc = torch.empty(max(n, 1), dtype=torch.int32, device=xt.device) if trace else None
        torch.cuda.synchronize(xt.device)
        mem = MEM_DEVICE
    else:
        xt = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        ct = None if color is None else np.ascontiguousarray(color, np.float32).reshape(-1, 3)
        assert ct is None or ct.shape == xt.shape
        n = xt.shape[0]
        xo = np.zeros((max(n, 1), 3), np.float32)
        co = np.zeros((max(n, 1), 3), np.float32) if ct is not None else None
        pv = np.zeros(max(n, 1), np.int32) if trace else None
        vc = np.zeros(max(n, 1), np.int32) if trace else None
        mem = MEM_HOST
    rows = C.c_int()
    _check(self.lib.svo_voxel_downsample(self._h, _ptr(xt), _ptr(ct), n, C.c_double(voxel_size), _ptr(xo), _ptr(co),
                                         C.byref(rows), _ptr(pv), _ptr(vc), mem))
    k = rows.value
    own = (lambda a: a) if mem == MEM_DEVICE else (lambda a: a.copy())
    res = (own(xo[:k]), own(co[:k]) if co is not None else None)
    return res + (own(pv[:n]), own(vc[:k])) if trace else res


# ---- stereo rectification and undistortion: stereoRectify -> initUndistortRectifyMap -> remap, undistortPoints ----------
CALIB_ZERO_DISPARITY = 1024
StereoRectification = collections.namedtuple("StereoRectification", "R1 R2 P1 P2 Q")


def _camera(K, D):
    K = np.ascontiguousarray(K, np.float64).reshape(3, 3)
    D = np.zeros(0) if D is None else np.ascontiguousarray(D, np.float64).reshape(-1)
    return K, D, len(D)


def _opt_matrix(M, shape):
    return None if M is None else np.ascontiguousarray(M, np.float64).reshape(shape)


def stereo_rectify(K1, D1, K2, D2, size, R, T, flags=CALIB_ZERO_DISPARITY, alpha=-1.0, new_size=(0, 0)):
    """``svo_stereo_rectify`` (host code, no context): cv::stereoRectify with alpha = -1 -> StereoRectification(R1, R2, P1, P2,
    Q), float64 matrices.  size: (w, h)."""
    K1, D1, n1 = _camera(K1, D1)
    K2, D2, n2 = _camera(K2, D2)
    R, T = np.ascontiguousarray(R, np.float64).reshape(3, 3), np.ascontiguousarray(T, np.float64).reshape(3)
    out = StereoRectification(np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 4)), np.zeros((3, 4)), np.zeros((4, 4)))
    _check(load().svo_stereo_rectify(_ptr(K1), _ptr(D1), n1, _ptr(K2), _ptr(D2), n2, int(size[0]), int(size[1]), _ptr(R), _ptr(T),
                                     int(flags), C.c_double(alpha), int(new_size[0]), int(new_size[1]), *[_ptr(a) for a in out]))
    return out


def undistort_points_host(xy, K, D, R=None, P=None):
    """``svo_undistort_points_host``: float32 points in, float64 points out; no context."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    K, D, nD = _camera(K, D)
    out = np.zeros((len(xy), 2), np.float64)
    _check(load().svo_undistort_points_host(_ptr(xy), len(xy), _ptr(K), _ptr(D), nD, _ptr(_opt_matrix(R, (3, 3))),
                                            _ptr(_opt_matrix(P, (3, 4))), _ptr(out)))
    return out


class RectifyMap(_Handle):
    """A fixed-point rectify map on the device (``svo_rectify_map``): ``Context.rectify_map`` / ``rectify_map_from_float``."""
    _destroy, _destroy_takes_ctx = "svo_rectify_map_destroy", True

    def __init__(self, ctx, handle, size, src_size):
        self.ctx, self._h, self.size, self.src_size = ctx, handle, tuple(size), tuple(src_size)
        ctx._children.add(self)

    def get(self):
        """-> (xy [h, w, 2] int16, frac [h, w] uint16)"""
        w, h = self.size
        xy, frac = np.zeros((h, w, 2), np.int16), np.zeros((h, w), np.uint16)
        _check(self.ctx.lib.svo_rectify_map_get(self.ctx._h, self._h, _ptr(xy), _ptr(frac), MEM_HOST))
        return xy, frac


@_ctx_method
def rectify_map(self, K, D, R, P, size, src_size=None):
    """``svo_rectify_map_create``: initUndistortRectifyMap(K, D, R, P, size) -> RectifyMap.  R, P may be None (identity, K);
    P is 3 x 4 (or 3 x 3); src_size: the size of the images to sample, ``size`` when None."""
    K, D, nD = _camera(K, D)
    if P is not None:
        P = np.asarray(P, np.float64)
        P = np.ascontiguousarray(np.hstack([P, np.zeros((3, 1))]) if P.shape == (3, 3) else P.reshape(3, 4))
    src = tuple(size) if src_size is None else tuple(src_size)
    h = C.c_void_p()
    _check(self.lib.svo_rectify_map_create(self._h, _ptr(K), _ptr(D), nD, _ptr(_opt_matrix(R, (3, 3))), _ptr(P), int(size[0]),
                                           int(size[1]), int(src[0]), int(src[1]), C.byref(h)))
    return RectifyMap(self, h, size, src)


@_ctx_method
def rectify_map_from_float(self, mapx, mapy, src_size):
    """``svo_rectify_map_from_float``: a caller's float maps (h x w each; numpy arrays or device tensors) -> RectifyMap."""
    dev = _is_device(mapx)
    assert dev == _is_device(mapy), "mapx and mapy must live in the same memory"
    if dev:
        import torch

        mx, my = mapx.to(torch.float32).contiguous(), mapy.to(torch.float32).contiguous()
        torch.cuda.synchronize(mx.device)
    else:
        mx, my = np.ascontiguousarray(mapx, np.float32), np.ascontiguousarray(mapy, np.float32)
    assert mx.ndim == 2 and tuple(mx.shape) == tuple(my.shape)
    hh, ww = mx.shape
    h = C.c_void_p()
    _check(self.lib.svo_rectify_map_from_float(self._h, _ptr(mx), _ptr(my), int(ww), int(hh), int(src_size[0]), int(src_size[1]),
                                               _mem_of(dev), C.byref(h)))
    return RectifyMap(self, h, (ww, hh), src_size)


def _image_batch(images, src_size):
    """one image (h x w or h x w x c) or a batch (n x h x w, n x h x w x c) of a map's source size -> (array, n, c, the leading
    shape of the result, device).  A 3-D array whose LAST two axes are the source size is a grey batch; only otherwise is it one
    image with channels (the two readings coincide only for a 1 x 1 or 3 x 3 source)."""
    dev = _is_device(images)
    a = images.contiguous() if dev else np.ascontiguousarray(images, np.uint8)
    sw, sh = src_size
    shape = tuple(a.shape)
    if len(shape) == 2:
        lead, n, c, hw = (), 1, 1, shape
    elif len(shape) == 3 and shape[1:] == (sh, sw):
        lead, n, c, hw = (shape[0],), shape[0], 1, shape[1:]
    elif len(shape) == 3:
        lead, n, c, hw = (), 1, shape[2], shape[:2]
    else:
        lead, n, c, hw = (shape[0],), shape[0], shape[3], shape[1:3]
    assert len(shape) <= 4 and hw == (sh, sw) and c in (1, 3), f"images must be {sh} x {sw} with 1 or 3 channels, the map's source size"
    if dev:
        import torch

        assert a.dtype == torch.uint8
    return a, n, c, (lead, len(shape) - len(lead) == 3), dev


def _remap_shape(lead_ch, size, c):
    lead, with_channels = lead_ch
    return lead + (size[1], size[0]) + ((c,) if with_channels else ())


@_ctx_method
def remap(self, map, images, border_value=0, mem=None):
    """``svo_remap_batch``: cv::remap(INTER_LINEAR, BORDER_CONSTANT) of one image or a batch of 1..16 (numpy arrays or device
    tensors, uint8, grey or 3 interleaved channels) through ``map`` -> images of the map's size with the same leading shape."""
    a, n, c, lead, dev = _image_batch(images, map.src_size)
    if mem is not None:
        assert (mem == MEM_DEVICE) == dev
    oshape = _remap_shape(lead, map.size, c)
    if dev:
        import torch

        out = torch.empty(oshape, dtype=torch.uint8, device=a.device)
        torch.cuda.synchronize(a.device)
    else:
        out = np.zeros(oshape, np.uint8)
    _check(self.lib.svo_remap_batch(self._h, map._h, _ptr(a), n, c, int(border_value), _ptr(out), _mem_of(dev)))
    return out


@_ctx_method
def rectify_pairs(self, map_left, map_right, lefts, rights, border_value=0, mem=None):
    """``svo_rectify_pairs``: both images of 1..16 stereo pairs through their maps in one launch -> (lefts, rights) rectified."""
    a, n, c, lead, dev = _image_batch(lefts, map_left.src_size)
    b, n2, c2, _, dev2 = _image_batch(rights, map_right.src_size)
    assert (n, c, dev) == (n2, c2, dev2), "lefts and rights must pair up and live in the same memory"
    if mem is not None:
        assert (mem == MEM_DEVICE) == dev
    oshape = _remap_shape(lead, map_left.size, c)
    if dev:
        import torch

        ol, orr = torch.empty(oshape, dtype=torch.uint8, device=a.device), torch.empty(oshape, dtype=torch.uint8, device=a.device)
        torch.cuda.synchronize(a.device)
    else:
        ol, orr = np.zeros(oshape, np.uint8), np.zeros(oshape, np.uint8)
    _check(self.lib.svo_rectify_pairs(self._h, map_left._h, map_right._h, _ptr(a), _ptr(b), n, c, int(border_value), _ptr(ol),
                                      _ptr(orr), _mem_of(dev)))
    return ol, orr


@_ctx_method
def undistort_points(self, xy, K, D, R=None, P=None, mem=None):
    """``svo_undistort_points``: cv::undistortPoints on n x 2 float32 points (a numpy array, or a device tensor which gives a
    device tensor back) -> n x 2 float32."""
    dev = _is_device(xy)
    if mem is not None:
        assert (mem == MEM_DEVICE) == dev
    K, D, nD = _camera(K, D)
    if dev:
        import torch

        pts = xy.reshape(-1, 2).to(torch.float32).contiguous()
        out = torch.empty_like(pts)
        torch.cuda.synchronize(pts.device)
    else:
        pts = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.zeros_like(pts)
    _check(self.lib.svo_undistort_points(self._h, _ptr(pts), int(pts.shape[0]), _ptr(K), _ptr(D), nD, _ptr(_opt_matrix(R, (3, 3))),
                                         _ptr(_opt_matrix(P, (3, 4))), _ptr(out), _mem_of(dev)))
    return out


# ---- two-view geometry: findEssentialMat / recoverPose (StereoProcess::monocularTriangulate) ----------------------
def _problem_set(p1, p2, K):
    """one problem (p1, p2: n x 2 arrays or device tensors, K: 4 numbers) or lists of them -> (p1 and p2 back to back,
    host offsets, host K4, single, device)"""
    single = not isinstance(p1, (list, tuple))
    p1s, p2s = ([p1], [p2]) if single else (list(p1), list(p2))
    assert len(p1s) == len(p2s) and 1 <= len(p1s) <= 16, "1 to 16 problems per call"
    Ks = [K] * len(p1s) if np.asarray(K, np.float64).size == 4 else list(K)
    assert len(Ks) == len(p1s)
    K4 = np.ascontiguousarray(np.concatenate([np.asarray(k, np.float64).reshape(4) for k in Ks]))
    dev = _is_device(p1s[0])
    sizes = [int(np.prod(a.shape)) // 2 for a in p1s]
    assert sizes == [int(np.prod(a.shape)) // 2 for a in p2s], "p1 and p2 must pair up"
    offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]), np.int32)
    if dev:
        import torch

        assert all(_is_device(a) for a in p1s + p2s), "all point arrays must live in the same memory"
        a = torch.cat([x.reshape(-1, 2).to(torch.float32) for x in p1s]).contiguous()
        b = torch.cat([x.reshape(-1, 2).to(torch.float32) for x in p2s]).contiguous()
    else:
        a = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 2) for x in p1s]))
        b = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 2) for x in p2s]))
    return a, b, offsets, K4, single, dev


@_ctx_method
def essential_5pt(self, x1n, x2n):
    """``svo_essential_5pt``: the five-point solver on s samples of normalised coordinates (s x 5 x 2 each) ->
    (E: s x 10 x 3 x 3, the first nsol[k] valid; nsol: s ints)."""
    x1 = np.ascontiguousarray(x1n, np.float64).reshape(-1, 5, 2)
    x2 = np.ascontiguousarray(x2n, np.float64).reshape(-1, 5, 2)
    assert x1.shape == x2.shape
    s = x1.shape[0]
    E = np.zeros((s, 10, 3, 3))
    nsol = np.zeros(s, np.int32)
    _check(self.lib.svo_essential_5pt(self._h, _ptr(x1), _ptr(x2), s, _ptr(E), _ptr(nsol), MEM_HOST))
    return E, nsol


@_ctx_method
def find_essential(self, p1, p2, K, threshold=1.0, confidence=0.99, max_iters=1000, seed=0):
    """``svo_find_essential`` (cv::findEssentialMat, RANSAC): one problem -- p1, p2 (n x 2 pixels), K = (fx, fy, cx, cy)
    -- or lists of up to 16 problems (K one for all or one per problem).  numpy arrays, or device tensors whose masks
    come back as device tensors.  Per problem -> (E: m x 3 x 3, mask: n uint8, inlier count, iterations run)."""
    a, b, offsets, K4, single, dev = _problem_set(p1, p2, K)
    nprob, total = len(offsets) - 1, int(offsets[-1])
    args = (C.c_double(threshold), C.c_double(confidence), int(max_iters), C.c_uint64(seed))
    if dev:
        import torch

        mask = torch.empty(max(total, 1), dtype=torch.uint8, device=a.device)
        E = torch.zeros((nprob, 10, 9), dtype=torch.float64, device=a.device)
        ints = torch.zeros((3, nprob), dtype=torch.int32, device=a.device)
        torch.cuda.synchronize(a.device)
        _check(self.lib.svo_find_essential(self._h, _ptr(a), _ptr(b), _ptr(offsets), nprob, _ptr(K4), *args, _ptr(mask),
                                           _ptr(E), _ptr(ints[0]), _ptr(ints[1]), _ptr(ints[2]), MEM_DEVICE))
        _check(self.lib.svo_ctx_sync(self._h))
        E, ints = E.cpu().numpy(), ints.cpu().numpy()
    else:
        mask = np.zeros(max(total, 1), np.uint8)
        E = np.zeros((nprob, 10, 9))
        ints = np.zeros((3, nprob), np.int32)
        _check(self.lib.svo_find_essential(self._h, _ptr(a), _ptr(b), _ptr(offsets), nprob, _ptr(K4), *args, _ptr(mask),
                                           _ptr(E), _ptr(ints[0]), _ptr(ints[1]), _ptr(ints[2]), MEM_HOST))
    out = [(E[k, :ints[0, k]].reshape(-1, 3, 3), mask[offsets[k]:offsets[k + 1]], int(ints[1, k]), int(ints[2, k]))
           for k in range(nprob)]
    return out[0] if single else out


@_ctx_method
def recover_pose(self, E, p1, p2, K, distance_thresh=50.0, mask=None):
    """``svo_recover_pose`` (cv::recoverPose): one problem -- E (3 x 3), p1, p2 (n x 2 pixels), K = (fx, fy, cx, cy),
    mask (n, optional: ANDed in) -- or lists of up to 16.  Host arrays -> per problem (R, t (3,), good count, the chosen
    candidate's mask)."""
    a, b, offsets, K4, single, dev = _problem_set(p1, p2, K)
    assert not dev, "recover_pose takes host arrays"
    nprob, total = len(offsets) - 1, int(offsets[-1])
    Es = [E] if single else list(E)
    assert len(Es) == nprob
    E9 = np.ascontiguousarray(np.concatenate([np.asarray(e, np.float64).reshape(9) for e in Es]))
    masks = [mask] if single else (list(mask) if mask is not None else [None] * nprob)
    m = np.ones(max(total, 1), np.uint8)
    for k, mk in enumerate(masks):
        if mk is not None:
            m[offsets[k]:offsets[k + 1]] = np.asarray(mk, np.uint8).reshape(-1)
    R, t, good = np.zeros((nprob, 3, 3)), np.zeros((nprob, 3)), np.zeros(nprob, np.int32)
    _check(self.lib.svo_recover_pose(self._h, _ptr(E9), _ptr(a), _ptr(b), _ptr(offsets), nprob, _ptr(K4),
                                     C.c_double(distance_thresh), _ptr(m), _ptr(R), _ptr(t), _ptr(good), MEM_HOST))
    out = [(R[k], t[k], int(good[k]), m[offsets[k]:offsets[k + 1]].copy()) for k in range(nprob)]
    return out[0] if single else out


def decompose_essential(E):
    """``svo_decompose_essential`` (cv::decomposeEssentialMat, host) -> (R1, R2, t)."""
    e = np.ascontiguousarray(E, np.float64).reshape(9)
    R1, R2, t = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3)
    _check(load().svo_decompose_essential(_ptr(e), _ptr(R1), _ptr(R2), _ptr(t)))
    return R1, R2, t


# ---- planar two-view geometry: findHomography / decomposeHomographyMat and the pose they give ---------------------
_NO_K = (1.0, 1.0, 0.0, 0.0)


@_ctx_method
def homography_4pt(self, x1, x2):
    """``svo_homography_4pt``: the minimal solver on s 4-samples (s x 4 x 2 each, x2 ~ H x1) -> (H: s x 3 x 3 with h8 = 1,
    zero where not ok; ok: s ints)."""
    x1 = np.ascontiguousarray(x1, np.float64).reshape(-1, 4, 2)
    x2 = np.ascontiguousarray(x2, np.float64).reshape(-1, 4, 2)
    assert x1.shape == x2.shape
    s = x1.shape[0]
    H = np.zeros((s, 3, 3))
    ok = np.zeros(s, np.int32)
    _check(self.lib.svo_homography_4pt(self._h, _ptr(x1), _ptr(x2), s, _ptr(H), _ptr(ok), MEM_HOST))
    return H, ok


@_ctx_method
def find_homography(self, p1, p2, threshold=3.0, confidence=0.995, max_iters=2000, seed=0):
    """``svo_find_homography`` (cv::findHomography, RANSAC): one problem -- p1, p2 (n x 2 pixels) -- or lists of up to 16
    problems.  numpy arrays, or device tensors whose masks come back as device tensors.  Per problem -> (H: 3 x 3 with
    h8 = 1, zero without a model; mask: n uint8; inlier count; iterations run)."""
    a, b, offsets, _, single, dev = _problem_set(p1, p2, _NO_K)
    nprob, total = len(offsets) - 1, int(offsets[-1])
    args = (C.c_double(threshold), C.c_double(confidence), int(max_iters), C.c_uint64(seed))
    if dev:
        import torch

        mask = torch.empty(max(total, 1), dtype=torch.uint8, device=a.device)
        H = torch.zeros((nprob, 9), dtype=torch.float64, device=a.device)
        ints = torch.zeros((2, nprob), dtype=torch.int32, device=a.device)
        torch.cuda.synchronize(a.device)
        _check(self.lib.svo_find_homography(self._h, _ptr(a), _ptr(b), _ptr(offsets), nprob, *args, _ptr(mask), _ptr(H),
                                            _ptr(ints[0]), _ptr(ints[1]), MEM_DEVICE))
        _check(self.lib.svo_ctx_sync(self._h))
        H, ints = H.cpu().numpy(), ints.cpu().numpy()
    else:
        mask = np.zeros(max(total, 1), np.uint8)
        H = np.zeros((nprob, 9))
        ints = np.zeros((2, nprob), np.int32)
        _check(self.lib.svo_find_homography(self._h, _ptr(a), _ptr(b), _ptr(offsets), nprob, *args, _ptr(mask), _ptr(H),
                                            _ptr(ints[0]), _ptr(ints[1]), MEM_HOST))
    out = [(H[k].reshape(3, 3), mask[offsets[k]:offsets[k + 1]], int(ints[0, k]), int(ints[1, k])) for k in range(nprob)]
    return out[0] if single else out


@_ctx_method
def homography_pose(self, H, p1, p2, K, distance_thresh=50.0, mask=None):
    """``svo_homography_pose``: one problem -- H (3 x 3), p1, p2 (n x 2 pixels), K = (fx, fy, cx, cy), mask (n, optional:
    ANDed in) -- or lists of up to 16.  Host arrays -> per problem (R, t (3,: unit norm, zero for a pure rotation), n (3,),
    good4 (the four candidates' counts), the chosen candidate's mask)."""
    a, b, offsets, K4, single, dev = _problem_set(p1, p2, K)
    assert not dev, "homography_pose takes host arrays"
    nprob, total = len(offsets) - 1, int(offsets[-1])
    Hs = [H] if single else list(H)
    assert len(Hs) == nprob
    H9 = np.ascontiguousarray(np.concatenate([np.asarray(h, np.float64).reshape(9) for h in Hs]))
    masks = [mask] if single else (list(mask) if mask is not None else [None] * nprob)
    m = np.ones(max(total, 1), np.uint8)
    for k, mk in enumerate(masks):
        if mk is not None:
            m[offsets[k]:offsets[k + 1]] = np.asarray(mk, np.uint8).reshape(-1)
    R, t, n, good4 = np.zeros((nprob, 3, 3)), np.zeros((nprob, 3)), np.zeros((nprob, 3)), np.zeros((nprob, 4), np.int32)
    _check(self.lib.svo_homography_pose(self._h, _ptr(H9), _ptr(a), _ptr(b), _ptr(offsets), nprob, _ptr(K4),
                                        C.c_double(distance_thresh), _ptr(m), _ptr(R), _ptr(t), _ptr(n), _ptr(good4), MEM_HOST))
    out = [(R[k], t[k], n[k], [int(g) for g in good4[k]], m[offsets[k]:offsets[k + 1]].copy()) for k in range(nprob)]
    return out[0] if single else out


def decompose_homography(H, K):
    """``svo_decompose_homography`` (cv::decomposeHomographyMat, host) -> list of (R, t, n): none, one (a pure rotation)
    or four, in the header's order."""
    h = np.ascontiguousarray(H, np.float64).reshape(9)
    K4 = np.ascontiguousarray(K, np.float64).reshape(4)
    R, t, n, nsol = np.zeros((4, 3, 3)), np.zeros((4, 3)), np.zeros((4, 3)), C.c_int(0)
    _check(load().svo_decompose_homography(_ptr(h), _ptr(K4), _ptr(R), _ptr(t), _ptr(n), C.byref(nsol)))
    return [(R[k], t[k], n[k]) for k in range(nsol.value)]


# ---- descriptor matching: BFMatcher::knnMatch + the ratio test (src/triangulation.cpp:120-133) ----------------------
MATCH_L2_F32, MATCH_L2_U8, MATCH_HAMMING = 0, 1, 2


def _match_rows(a, norm):
    """descriptor rows for ``svo_knn_match`` -> (contiguous array or tensor, dim).  L2_F32: float32 rows.  L2_U8 / HAMMING: the
    bytes of the rows, whatever integer type holds them (ORB's n x 8 uint32 words are 32 bytes, or 8 words, per row)."""
    if _is_device(a):
        import torch

        a = a.contiguous()
        assert a.ndim == 2
        if norm == MATCH_L2_F32:
            assert a.dtype == torch.float32, "L2_F32 takes float32 rows"
            return a, int(a.shape[1])
        assert not a.dtype.is_floating_point, "L2_U8 / HAMMING take integer rows"
        row_bytes = int(a.shape[1]) * a.element_size()
    else:
        a = np.asarray(a)
        assert a.ndim == 2
        if norm == MATCH_L2_F32:
            a = np.ascontiguousarray(a, np.float32)
            return a, int(a.shape[1])
        assert a.dtype.kind in "ui", "L2_U8 / HAMMING take integer rows"
        a = np.ascontiguousarray(a)
        row_bytes = int(a.shape[1]) * a.itemsize
    if norm == MATCH_L2_U8:
        return a, row_bytes
    assert row_bytes % 4 == 0, "HAMMING rows are whole 32-bit words"
    return a, row_bytes // 4


@_ctx_method
def knn_match(self, query, train, k=2, norm=MATCH_L2_U8, q_offsets=None, t_offsets=None):
    """``svo_knn_match`` (cv::BFMatcher(norm, false).knnMatch): query / train descriptor rows (numpy arrays, or device
    tensors which give device tensors back) -> (idx [nq, k] int32, dist [nq, k] float32), best first, ties to the lower
    train index, missing slots -1 / inf.  q_offsets / t_offsets (p + 1 ints each): up to 16 independent problems over row
    ranges of the two arrays, train indices local to each; without them one problem over all rows."""
    q, dim = _match_rows(query, norm)
    t, dim_t = _match_rows(train, norm)
    assert dim == dim_t, "query and train rows differ in length"
    dev = _is_device(q)
    assert dev == _is_device(t), "query and train must live in the same memory"
    nq, nt = int(q.shape[0]), int(t.shape[0])
    qo = np.ascontiguousarray([0, nq] if q_offsets is None else q_offsets, np.int32)
    to = np.ascontiguousarray([0, nt] if t_offsets is None else t_offsets, np.int32)
    assert len(qo) == len(to) and len(qo) >= 2
    assert len(qo) < 2 or (int(qo[-1]) <= nq and int(to[-1]) <= nt), "offsets beyond the arrays"
    nprob = len(qo) - 1
    if dev:
        import torch

        idx = torch.full((nq, k), -1, dtype=torch.int32, device=q.device)
        dist = torch.full((nq, k), float("inf"), dtype=torch.float32, device=q.device)
        torch.cuda.synchronize(q.device)
        _check(self.lib.svo_knn_match(self._h, int(norm), _ptr(q), _ptr(t), dim, _ptr(qo), _ptr(to), nprob, int(k), _ptr(idx),
                                      _ptr(dist), MEM_DEVICE))
        _check(self.lib.svo_ctx_sync(self._h))
        return idx, dist
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float32)
    _check(self.lib.svo_knn_match(self._h, int(norm), _ptr(q), _ptr(t), dim, _ptr(qo), _ptr(to), nprob, int(k), _ptr(idx),
                                  _ptr(dist), MEM_HOST))
    return idx, dist


@_ctx_method
def ratio_pairs(self, idx, dist, xy_query, xy_train, ratio=0.8):
    """``svo_ratio_pairs`` (the loop of src/triangulation.cpp:127-133): idx / dist as ``knn_match`` returns them for one
    problem, xy_query / xy_train the key points (n x 2) -> (p1 [m, 2], p2 [m, 2], mask [nq] uint8).  numpy arrays, or
    device tensors which give device tensors back."""
    dev = _is_device(idx)
    assert all(_is_device(a) == dev for a in (dist, xy_query, xy_train)), "all arrays must live in the same memory"
    nq, k = int(idx.shape[0]), int(idx.shape[1])
    cnt = C.c_int()
    if dev:
        import torch

        i_, d_ = idx.to(torch.int32).contiguous(), dist.to(torch.float32).contiguous()
        xq = xy_query.to(torch.float32).reshape(-1, 2).contiguous()
        xt = xy_train.to(torch.float32).reshape(-1, 2).contiguous()
        assert xq.shape[0] == nq
        p1 = torch.zeros((max(nq, 1), 2), dtype=torch.float32, device=i_.device)
        p2 = torch.zeros_like(p1)
        mask = torch.zeros(max(nq, 1), dtype=torch.uint8, device=i_.device)
        torch.cuda.synchronize(i_.device)
        _check(self.lib.svo_ratio_pairs(self._h, _ptr(i_), _ptr(d_), nq, k, C.c_double(ratio), _ptr(xq), _ptr(xt), _ptr(p1),
                                        _ptr(p2), _ptr(mask), C.byref(cnt), MEM_DEVICE))
        _check(self.lib.svo_ctx_sync(self._h))
        return p1[:cnt.value], p2[:cnt.value], mask[:nq]
    i_, d_ = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(dist, np.float32)
    xq = np.ascontiguousarray(xy_query, np.float32).reshape(-1, 2)
    xt = np.ascontiguousarray(xy_train, np.float32).reshape(-1, 2)
    assert xq.shape[0] == nq and (nq == 0 or int(i_[:, 0].max()) < xt.shape[0])
    p1, p2 = np.zeros((max(nq, 1), 2), np.float32), np.zeros((max(nq, 1), 2), np.float32)
    mask = np.zeros(max(nq, 1), np.uint8)
    _check(self.lib.svo_ratio_pairs(self._h, _ptr(i_), _ptr(d_), nq, k, C.c_double(ratio), _ptr(xq), _ptr(xt), _ptr(p1), _ptr(p2),
                                    _ptr(mask), C.byref(cnt), MEM_HOST))
    return p1[:cnt.value].copy(), p2[:cnt.value].copy(), mask[:nq].copy()


# ---- cross-check, radius and masked matching (svo_match_cross, svo_radius_match, svo_knn_match_gated) -----------------
CROSS_MUTUAL, CROSS_CV = 0, 1
RADIUS_MAX_PER_QUERY = 8192


class MatchGate(C.Structure):
    """``svo_match_gate``: train row t is a candidate of query q when |y_q - y_t| <= dy_max and dx_min <= x_q - x_t <= dx_max."""
    _fields_ = [("dy_max", C.c_float), ("dx_min", C.c_float), ("dx_max", C.c_float)]


def _match_problem(query, train, norm, q_offsets, t_offsets):
    """the arguments the matching calls share -> (q, t, dim, device?, nq, nt, q_offsets, t_offsets, nprob)"""
    q, dim = _match_rows(query, norm)
    t, dim_t = _match_rows(train, norm)
    assert dim == dim_t, "query and train rows differ in length"
    dev = _is_device(q)
    assert dev == _is_device(t), "query and train must live in the same memory"
    nq, nt = int(q.shape[0]), int(t.shape[0])
    qo = np.ascontiguousarray([0, nq] if q_offsets is None else q_offsets, np.int32)
    to = np.ascontiguousarray([0, nt] if t_offsets is None else t_offsets, np.int32)
    assert len(qo) == len(to) and len(qo) >= 2
    assert int(qo[-1]) <= nq and int(to[-1]) <= nt, "offsets beyond the arrays"
    return q, t, dim, dev, nq, nt, qo, to, len(qo) - 1


def _same_memory(a, dev, dtype, what):
    """an auxiliary array of a matching call, contiguous, in the memory of the descriptors"""
    assert _is_device(a) == dev, f"{what} must live in the memory of the descriptors"
    if dev:
        import torch

        return a.to(getattr(torch, dtype)).contiguous()
    return np.ascontiguousarray(a, getattr(np, dtype))


@_ctx_method
def match_cross(self, query, train, norm=MATCH_L2_U8, mode=CROSS_MUTUAL, q_offsets=None, t_offsets=None):
    """``svo_match_cross`` (cv::BFMatcher(norm, true).match): -> (idx [nq] int32, dist [nq] float32), -1 / inf for a query without
    a partner.  ``CROSS_MUTUAL``: i and j are each other's best; ``CROSS_CV``: OpenCV 3.2's reverse-search-only update.  numpy
    arrays, or device tensors which give device tensors back; offsets as ``knn_match``."""
    q, t, dim, dev, nq, nt, qo, to, nprob = _match_problem(query, train, norm, q_offsets, t_offsets)
    if dev:
        import torch

        idx = torch.full((nq,), -1, dtype=torch.int32, device=q.device)
        dist = torch.full((nq,), float("inf"), dtype=torch.float32, device=q.device)
        torch.cuda.synchronize(q.device)
    else:
        idx, dist = np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32)
    _check(self.lib.svo_match_cross(self._h, int(norm), _ptr(q), _ptr(t), dim, _ptr(qo), _ptr(to), nprob, int(mode), _ptr(idx),
                                    _ptr(dist), _mem_of(dev)))
    if dev:
        _check(self.lib.svo_ctx_sync(self._h))
    return idx, dist


@_ctx_method
def radius_match(self, query, train, max_distance, norm=MATCH_L2_U8, capacity=None, q_offsets=None, t_offsets=None):
    """``svo_radius_match`` (cv::BFMatcher::radiusMatch) -> (row_offsets, idx, dist): query i of problem p owns
    ``idx[o[i]:o[i + 1]]`` with ``o = row_offsets[q_offsets[p] + p:]``, sorted by distance, ties to the lower train index.
    ``capacity`` (entries of idx / dist; default: every pair of one problem) too small, or a query with more than
    ``RADIUS_MAX_PER_QUERY`` matches, raises ``SvoError`` (``SVO_ERR_CAPACITY``) whose ``row_offsets`` / ``total`` attributes hold
    what would be needed.  numpy arrays, or device tensors which give device tensors back."""
    q, t, dim, dev, nq, nt, qo, to, nprob = _match_problem(query, train, norm, q_offsets, t_offsets)
    if capacity is None:
        capacity = int(np.sum(np.diff(qo).astype(np.int64) * np.diff(to).astype(np.int64)))
    capacity = int(capacity)
    n_off = int(qo[-1]) + nprob
    total = C.c_int(0)
    if dev:
        import torch

        off = torch.zeros(n_off, dtype=torch.int32, device=q.device)
        idx = torch.full((max(capacity, 1),), -1, dtype=torch.int32, device=q.device)
        dist = torch.full((max(capacity, 1),), float("inf"), dtype=torch.float32, device=q.device)
        torch.cuda.synchronize(q.device)
    else:
        off = np.zeros(n_off, np.int32)
        idx, dist = np.full(max(capacity, 1), -1, np.int32), np.full(max(capacity, 1), np.inf, np.float32)
    rc = self.lib.svo_radius_match(self._h, int(norm), _ptr(q), _ptr(t), dim, _ptr(qo), _ptr(to), nprob, C.c_float(max_distance),
                                   _ptr(off), _ptr(idx), _ptr(dist), capacity, C.byref(total), _mem_of(dev))
    if rc == SVO_ERR_CAPACITY and total.value > 0:
        err = SvoError(rc, load().svo_last_error().decode(errors="replace"))
        err.row_offsets, err.total = off, total.value
        raise err
    _check(rc)
    return off, idx[:total.value], dist[:total.value]


@_ctx_method
def knn_match_gated(self, query, train, k=2, norm=MATCH_L2_U8, mask=None, gate=None, xy_query=None, xy_train=None, q_offsets=None,
                    t_offsets=None):
    """``svo_knn_match_gated`` (knnMatch with a mask): ``knn_match`` over the allowed pairs only.  Either ``mask`` -- nonzero bytes
    allow; one problem: an nq x nt array, a batch: the problems' matrices flattened back to back -- or ``gate`` = (dy_max,
    dx_min, dx_max) with the key points ``xy_query`` / ``xy_train`` (n x 2): |y_q - y_t| <= dy_max and dx_min <= x_q - x_t <=
    dx_max.  numpy arrays, or device tensors which give device tensors back."""
    assert (mask is None) != (gate is None), "either a mask or a gate"
    q, t, dim, dev, nq, nt, qo, to, nprob = _match_problem(query, train, norm, q_offsets, t_offsets)
    m = xq = xt = g = None
    if mask is not None:
        m = _same_memory(mask, dev, "uint8", "mask").reshape(-1)
        need = int(np.sum(np.diff(qo).astype(np.int64) * np.diff(to).astype(np.int64)))
        assert int(m.shape[0]) == need, "the mask holds nq x nt bytes per problem"
        if need == 0:  # nothing to read: any address stands for the form
            m = np.zeros(1, np.uint8) if not dev else m.new_zeros(1)
    else:
        xq = _same_memory(xy_query, dev, "float32", "xy_query").reshape(-1, 2)
        xt = _same_memory(xy_train, dev, "float32", "xy_train").reshape(-1, 2)
        assert int(xq.shape[0]) == nq and int(xt.shape[0]) == nt, "a key point per descriptor row"
        if nq == 0 or nt == 0:
            xq = xq if nq else (np.zeros((1, 2), np.float32) if not dev else xq.new_zeros((1, 2)))
            xt = xt if nt else (np.zeros((1, 2), np.float32) if not dev else xt.new_zeros((1, 2)))
        g = gate if isinstance(gate, MatchGate) else MatchGate(*(float(v) for v in gate))
    if dev:
        import torch

        idx = torch.full((nq, k), -1, dtype=torch.int32, device=q.device)
        dist = torch.full((nq, k), float("inf"), dtype=torch.float32, device=q.device)
        torch.cuda.synchronize(q.device)
    else:
        idx, dist = np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, np.float32)
    _check(self.lib.svo_knn_match_gated(self._h, int(norm), _ptr(q), _ptr(t), dim, _ptr(qo), _ptr(to), nprob, int(k), _ptr(m),
                                        _ptr(xq), _ptr(xt), C.byref(g) if g is not None else None, _ptr(idx), _ptr(dist),
                                        _mem_of(dev)))
    if dev:
        _check(self.lib.svo_ctx_sync(self._h))
    return idx, dist


@_ctx_method
def pnp_ransac(self, obj, img, K4, iterations=100, reproj_err=1.0, confidence=0.99, seed=0):
    obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
    n = obj.shape[0]
    rvec, tvec = np.zeros(3), np.zeros(3)
    inl = np.zeros(max(n, 1), np.int32)
    cnt, iters = C.c_int(), C.c_int()
    _check(self.lib.svo_pnp_ransac(self._h, _ptr(obj), _ptr(img), n, _ptr(np.ascontiguousarray(K4, np.float64)),
                                   iterations, C.c_double(reproj_err), C.c_double(confidence), C.c_uint64(seed),
                                   _ptr(rvec), _ptr(tvec), _ptr(inl), C.byref(cnt), C.byref(iters), MEM_HOST))
    return cnt.value, rvec, tvec, inl[:cnt.value].copy(), iters.value


@_ctx_method
def pnp_ladder(self, obj_f, img_f, obj_s, img_s, K4, seed=0):
    """The older ladder's pose stage (``svo_pnp_ladder``) -> (rc, rvec, tvec, n_inliers, rung)."""
    of = np.ascontiguousarray(obj_f, np.float32).reshape(-1, 3)
    uf = np.ascontiguousarray(img_f, np.float32).reshape(-1, 2)
    os_ = np.ascontiguousarray(obj_s, np.float32).reshape(-1, 3)
    us = np.ascontiguousarray(img_s, np.float32).reshape(-1, 2)
    rvec, tvec, ninl, rung = np.zeros(3), np.zeros(3), C.c_int(), C.c_int()
    rc = self.lib.svo_pnp_ladder(self._h, _ptr(of), _ptr(uf), len(of), _ptr(os_), _ptr(us), len(os_),
                                 _ptr(np.ascontiguousarray(K4, np.float64)), C.c_uint64(seed), _ptr(rvec), _ptr(tvec),
                                 C.byref(ninl), C.byref(rung), MEM_HOST)
    if rc not in (SVO_OK, SVO_ERR_TRACKING_LOST):
        _check(rc)
    return rc, rvec, tvec, ninl.value, rung.value


@_ctx_method
def solve_pnp(self, obj, img, K4):
    """cv::solvePnP (ITERATIVE, no guess; src/bundleAdjust.cpp:470-477) -> (rvec, tvec, rms)."""
    obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
    rvec, tvec, rms = np.zeros(3), np.zeros(3), C.c_double()
    _check(self.lib.svo_solve_pnp(self._h, _ptr(obj), _ptr(img), obj.shape[0], _ptr(np.ascontiguousarray(K4, np.float64)),
                                  _ptr(rvec), _ptr(tvec), C.byref(rms), MEM_HOST))
    return rvec, tvec, rms.value


@_ctx_method
def ba_3d2d(self, pts2d, pts3d, K4, R, t, iterations=10):
    """visualOdometry::BundleAdjust3d2d (src/bundleAdjust.cpp:551-613) -> (t, R, points, info)."""
    p2 = np.ascontiguousarray(pts2d, np.float32).reshape(-1, 2)
    p3 = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
    n = p2.shape[0]
    tio = np.array(t, np.float64).reshape(3).copy()
    Rout, Xout, info = np.zeros((3, 3)), np.zeros((n, 3)), np.zeros(5)
    _check(self.lib.svo_ba_3d2d(self._h, _ptr(p2), _ptr(p3), n, _ptr(np.ascontiguousarray(K4, np.float64)),
                                _ptr(np.ascontiguousarray(R, np.float64).reshape(3, 3)), _ptr(tio), int(iterations),
                                _ptr(Rout), _ptr(Xout), _ptr(info), MEM_HOST))
    return tio, Rout, Xout, dict(chi2_before=info[0], chi2_after=info[1], lambda_final=info[2],
                                 iterations=int(info[3]), trials=int(info[4]))


class ba_window_params(C.Structure):
    """``svo_ba_window_params``; ``ba_window_params.default()`` holds the library's defaults."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double),
                ("iterations", C.c_int), ("huber_mono", C.c_double), ("huber_stereo", C.c_double)]

    @classmethod
    def default(cls, **kw):
        _known_fields(cls, "svo_ba_window_params", kw)
        return _make_params(cls, "svo_ba_window_default_params", kw)


@_ctx_method
def ba_window(self, poses, fixed, pts3d, obs_start, obs_pose, obs_uvr, params=None, mem=MEM_HOST):
    """Windowed bundle adjustment (``svo_ba_window``) -> (poses (P, 12), points (N, 3), per-observation chi2, info).  ``poses``: R9 | t3
    per pose, world -> camera; ``fixed``: one byte per pose; the observations CSR by point.  ``pts3d``, ``obs_start``, ``obs_pose``
    and ``obs_uvr`` follow ``mem`` (device: tensors or addresses, with ``obs_start`` readable for its sizes only through the
    library); ``params``: a ``ba_window_params`` or a dict of its fields."""
    params = _as_params(ba_window_params, ba_window_params.default, params)
    P = np.array(poses, np.float64).reshape(-1, 12).copy()
    fx = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    assert fx.shape[0] == P.shape[0]
    if mem == MEM_HOST:
        pts3d = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
        obs_start = np.ascontiguousarray(obs_start, np.int32).reshape(-1)
        obs_pose = np.ascontiguousarray(obs_pose, np.int32).reshape(-1)
        obs_uvr = np.ascontiguousarray(obs_uvr, np.float32).reshape(-1, 3)
        n, n_obs = pts3d.shape[0], obs_pose.shape[0]
        assert obs_start.shape[0] == n + 1 and obs_uvr.shape[0] == n_obs and (n_obs == 0 or int(obs_start.max()) <= n_obs)
    else:
        n, n_obs = int(obs_start.shape[0]) - 1, int(obs_pose.shape[0])
    Xout, chi, info = np.zeros((n, 3)), np.zeros(n_obs), np.zeros(6)
    _check(self.lib.svo_ba_window(self._h, C.byref(params), P.shape[0], _ptr(P), _ptr(fx), n, _ptr(pts3d), _ptr(obs_start),
                                  _ptr(obs_pose), _ptr(obs_uvr), _ptr(Xout), _ptr(chi), _ptr(info), mem))
    return P, Xout, chi, dict(chi2_before=info[0], chi2_after=info[1], lambda_final=info[2], iterations=int(info[3]),
                              trials=int(info[4]), observations=int(info[5]))


class VoParams(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("baseline", C.c_double), ("grid_step", C.c_int), ("anms_keep", C.c_int),
                ("keyframe_min_inliers", C.c_int), ("f_thr_stereo", C.c_double),
                ("f_thr_temporal", C.c_double), ("seed", C.c_uint64), ("policy", C.c_int),
                ("pnp_retry_below", C.c_int), ("pnp_lost_below", C.c_int)]


class VisualOdometry(_Handle):
    """The front-end frame loop on one GPU (``svo_vo``), mirroring visualSLAM::initSequence
    (src/VisualSLAM.cpp:11-169).  Images: numpy (H, W, C) uint8 or device tensors."""
    _destroy = "svo_vo_destroy"

    def __init__(self, ctx: Context, w, h, c, grid_step=30, anms_keep=0, keyframe_min_inliers=200, seed=0,
                 K4=None, baseline=None, policy=0, pnp_retry_below=None, pnp_lost_below=None):
        self.ctx = ctx
        self.prm = _make_params(VoParams, "svo_vo_default_params", dict(
            grid_step=grid_step, anms_keep=anms_keep, keyframe_min_inliers=keyframe_min_inliers, seed=seed, policy=policy))
        if pnp_retry_below is not None:
            self.prm.pnp_retry_below = pnp_retry_below
        if pnp_lost_below is not None:
            self.prm.pnp_lost_below = pnp_lost_below
        if K4 is not None:
            self.prm.fx, self.prm.fy, self.prm.cx, self.prm.cy = K4
        if baseline is not None:
            self.prm.baseline = baseline
        self._h = C.c_void_p()
        _check(ctx.lib.svo_vo_create(ctx._h, C.byref(self.prm), w, h, c, C.byref(self._h)))
        ctx._children.add(self)

    @staticmethod
    def _mem(img):
        """numpy arrays and CPU torch tensors (pinned or not) are host memory, CUDA tensors / raw addresses device memory"""
        if isinstance(img, np.ndarray):
            return MEM_HOST
        if hasattr(img, "is_cuda"):
            return MEM_DEVICE if img.is_cuda else MEM_HOST
        return MEM_DEVICE

    def init(self, left, right):
        n = C.c_int()
        _check(self.ctx.lib.svo_vo_init(self._h, _ptr(left), _ptr(right), self._mem(left), C.byref(n)))
        return n.value

    def localize(self, left):
        R, t = np.zeros((3, 3)), np.zeros(3)
        ninl, ntrk = C.c_int(), C.c_int()
        rc = self.ctx.lib.svo_vo_localize(self._h, _ptr(left), self._mem(left), _ptr(R), _ptr(t), C.byref(ninl),
                                          C.byref(ntrk))
        if rc not in (SVO_OK, SVO_ERR_TRACKING_LOST):
            _check(rc)
        return rc, R, t, ninl.value, ntrk.value

    def update(self, right, R, t, n_inliers, force_keyframe=False):
        kf = C.c_int()
        mem = MEM_HOST if right is None else self._mem(right)
        _check(self.ctx.lib.svo_vo_update(self._h, _ptr(right), mem, _ptr(np.ascontiguousarray(R, np.float64)),
                                          _ptr(np.ascontiguousarray(t, np.float64)), n_inliers,
                                          int(force_keyframe), C.byref(kf)))
        return bool(kf.value)

    def track(self, left, right, force_keyframe=False):
        rc, R, t, ninl, ntrk = self.localize(left)
        if rc:
            return rc, R, t, ninl, False, ntrk
        kf = self.update(right, R, t, ninl, force_keyframe)
        return rc, R, t, ninl, kf, ntrk

    STAGE_NAMES = ("frame_period", "filters", "tracking_launch", "wait_for_decision", "pnp_stream_lag",
                   "pnp_to_decision", "keyframe_refine_handover", "stereo_stream_lag", "stereo_path")

    def set_stage_stamps(self, enable: bool = True):
        _check(self.ctx.lib.svo_vo_set_stage_stamps(self._h, int(enable)))

    def stage_us(self):
        """Mean stage intervals (microseconds) of the last pipelined run with stamps on -> (dict, frames averaged)."""
        us = (C.c_double * len(self.STAGE_NAMES))()
        n = C.c_int()
        _check(self.ctx.lib.svo_vo_get_stage_us(self._h, us, len(self.STAGE_NAMES), C.byref(n)))
        return {k: float(v) for k, v in zip(self.STAGE_NAMES, us)}, n.value

    def run_chunk(self, lefts, rights, pipeline: bool = True):
        """Consecutive frames without returning to Python in between (``svo_vo_run_chunk``).
        Returns (rc, n_done, R[n,3,3], t[n,3], inliers[n], tracked[n], keyframe[n])."""
        n = len(lefts)
        mem = self._mem(lefts[0])
        PtrArr = C.c_void_p * n
        la = PtrArr(*[_ptr(x).value for x in lefts])
        ra = PtrArr(*[_ptr(x).value for x in rights])
        R, t = np.zeros((n, 3, 3)), np.zeros((n, 3))
        inl, trk = np.zeros(n, np.int32), np.zeros(n, np.int32)
        kf = np.zeros(n, np.uint8)
        done = C.c_int()
        rc = self.ctx.lib.svo_vo_run_chunk(self._h, la, ra, n, mem, int(bool(pipeline)), _ptr(R), _ptr(t), _ptr(inl),
                                           _ptr(trk), _ptr(kf), C.byref(done))
        if rc not in (SVO_OK, SVO_ERR_TRACKING_LOST):
            _check(rc)
        return rc, done.value, R, t, inl, trk, kf.astype(bool)

    def keyframe_cloud(self):
        """The last keyframe's camera-frame cloud (``untransformed``) -> (n, 3) float32."""
        cap = self.ctx.lib.svo_vo_capacity(self._h)
        a = np.zeros((cap, 3), np.float32)
        n = C.c_int()
        _check(self.ctx.lib.svo_vo_get_keyframe_cloud(self._h, _ptr(a), cap, C.byref(n), MEM_HOST))
        return a[:n.value]

    def keyframe_colors(self):
        """``colors`` of the last keyframe (B, G, R floats per point, point for point with keyframe_cloud())."""
        cap = self.ctx.lib.svo_vo_capacity(self._h)
        a = np.zeros((cap, 3), np.float32)
        n = C.c_int()
        _check(self.ctx.lib.svo_vo_get_keyframe_colors(self._h, _ptr(a), cap, C.byref(n), MEM_HOST))
        return a[:n.value]

    def reference(self):
        cap = self.ctx.lib.svo_vo_capacity(self._h)
        a, b = np.zeros((cap, 2), np.float32), np.zeros((cap, 3), np.float32)
        n = C.c_int()
        _check(self.ctx.lib.svo_vo_get_reference(self._h, _ptr(a), _ptr(b), cap, C.byref(n), MEM_HOST))
        return a[:n.value], b[:n.value]


# ---- data formats either side of the path (host code in libsvo_hip.so, no GPU needed) -----------
def read_kitti_poses(path):
    """-> (R[n,3,3], t[n,3]) of a KITTI odometry pose file."""
    lib = load()
    n = C.c_int()
    _check(lib.svo_io_read_kitti_poses(str(path).encode(), None, 0, C.byref(n)))
    buf = np.zeros((max(n.value, 1), 12))
    _check(lib.svo_io_read_kitti_poses(str(path).encode(), _ptr(buf), n.value, C.byref(n)))
    Rt = buf[:n.value].reshape(-1, 3, 4)
    return Rt[:, :, :3].copy(), Rt[:, :, 3].copy()


def write_kitti_poses(path, R, t):
    R = np.ascontiguousarray(R, np.float64).reshape(-1, 9)
    t = np.ascontiguousarray(t, np.float64).reshape(-1, 3)
    _check(load().svo_io_write_kitti_poses(str(path).encode(), _ptr(R), _ptr(t), len(R)))


def trajectory_csv(path, rows8, create=True):
    rows8 = np.ascontiguousarray(rows8, np.float32).reshape(-1, 8)
    _check(load().svo_io_trajectory_csv(str(path).encode(), _ptr(rows8), len(rows8), int(bool(create))))


def ate_rmse(t_est, t_gt):
    a = np.ascontiguousarray(t_est, np.float64).reshape(-1, 3)
    b = np.ascontiguousarray(t_gt, np.float64).reshape(-1, 3)
    out = C.c_double()
    _check(load().svo_eval_ate_rmse(_ptr(a), _ptr(b), len(a), C.byref(out)))
    return out.value


def rpe(R_est, t_est, R_gt, t_gt, delta=1):
    """-> (translation RMSE, rotation RMSE in rad) over frame pairs (i, i + delta)."""
    Re = np.ascontiguousarray(R_est, np.float64).reshape(-1, 9)
    Rg = np.ascontiguousarray(R_gt, np.float64).reshape(-1, 9)
    te = np.ascontiguousarray(t_est, np.float64).reshape(-1, 3)
    tg = np.ascontiguousarray(t_gt, np.float64).reshape(-1, 3)
    a, b = C.c_double(), C.c_double()
    _check(load().svo_eval_rpe(_ptr(Re), _ptr(te), _ptr(Rg), _ptr(tg), len(Re), int(delta), C.byref(a), C.byref(b)))
    return a.value, b.value


def ros_map_points(xyz, bgr=None):
    """rosPublish's cloud (src/rosFuncs.cpp:49-62) -> (xyz', rgb uint8 or None)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    col = None if bgr is None else np.ascontiguousarray(bgr, np.float32).reshape(-1, 3)
    xo = np.zeros((max(len(xyz), 1), 3), np.float32)
    co = np.zeros((max(len(xyz), 1), 3), np.uint8)
    k = load().svo_ros_map_points(_ptr(xyz), _ptr(col), len(xyz), _ptr(xo), _ptr(co) if col is not None else _ptr(None))
    if k < 0:
        _check(k)
    return xo[:k].copy(), (co[:k].copy() if col is not None else None)


def ros_pose(R, t):
    pos, quat = np.zeros(3), np.zeros(4)
    _check(load().svo_ros_pose(_ptr(np.ascontiguousarray(R, np.float64)), _ptr(np.ascontiguousarray(t, np.float64)),
                               _ptr(pos), _ptr(quat)))
    return pos, quat


def write_ply(path, xyz, rgb=None):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    col = None if rgb is None else np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    _check(load().svo_io_write_ply(str(path).encode(), _ptr(xyz), _ptr(col), len(xyz)))


class ShardComm:
    """The chunk-sharded batch's one collective behind the C ABI (``svo_shard_*``): an RCCL communicator of one rank
    per GPU and the all-gather of chunk-boundary poses.  ``id128``: bytes from :func:`shard_unique_id` of ONE rank."""

    def __init__(self, ctx: "Context", rank: int, nranks: int, id128: bytes):
        self.ctx = ctx
        self._h = C.c_void_p()
        buf = (C.c_char * 128).from_buffer_copy(id128)
        _check(ctx.lib.svo_shard_comm_create(ctx._h, rank, nranks, buf, C.byref(self._h)))
        self.rank, self.nranks = rank, nranks

    def allgather_boundaries(self, pairs):
        """pairs: this rank's [(R, t)] chunk-boundary poses -> all ranks' in global chunk order."""
        loc = np.ascontiguousarray([np.r_[np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel()]
                                    for R, t in pairs], np.float64)
        out = np.zeros((self.nranks * len(pairs), 12))
        _check(self.ctx.lib.svo_shard_allgather_boundaries(self._h, _ptr(loc), len(pairs), _ptr(out)))
        return [(row[:9].reshape(3, 3).copy(), row[9:].copy()) for row in out]

    def allgather_bytes(self, mine: np.ndarray) -> np.ndarray:
        """``svo_shard_allgather_bytes``: a uint8 array of the same length on every rank -> (nranks, len) uint8."""
        mine = np.ascontiguousarray(mine, np.uint8).reshape(-1)
        out = np.zeros((self.nranks, len(mine)), np.uint8)
        self.ctx.lib.svo_shard_allgather_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        _check(self.ctx.lib.svo_shard_allgather_bytes(self._h, _ptr(mine), C.c_size_t(len(mine)), _ptr(out)))
        return out

    def close(self):
        if self._h:
            self.ctx.lib.svo_shard_comm_destroy(self._h)
            self._h = C.c_void_p()


def shard_unique_id() -> bytes:
    buf = (C.c_char * 128)()
    _check(load().svo_shard_unique_id(buf))
    return bytes(buf.raw)


def shard_prefix_starts(boundaries):
    """``svo_shard_prefix_starts``: [(R, t)] boundaries of all chunks -> global pose of every chunk's first frame."""
    b = np.ascontiguousarray([np.r_[np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel()]
                              for R, t in boundaries], np.float64)
    out = np.zeros_like(b)
    _check(load().svo_shard_prefix_starts(_ptr(b), len(boundaries), _ptr(out)))
    return [(row[:9].reshape(3, 3).copy(), row[9:].copy()) for row in out]


def shard_rebase(start, poses):
    """``svo_shard_rebase``: chunk-local [(R, t)] -> global, given the chunk's start pose (R, t)."""
    s12 = np.r_[np.asarray(start[0], np.float64).ravel(), np.asarray(start[1], np.float64).ravel()]
    p = np.ascontiguousarray([np.r_[np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel()]
                              for R, t in poses], np.float64).reshape(-1, 12)
    _check(load().svo_shard_rebase(_ptr(s12), _ptr(p), len(poses)))
    return [(row[:9].reshape(3, 3).copy(), row[9:].copy()) for row in p]


class _ChunkJob(C.Structure):
    _fields_ = [("vo", C.c_void_p), ("lefts", C.c_void_p), ("rights", C.c_void_p), ("n_frames", C.c_int),
                ("mem", C.c_int), ("pipeline", C.c_int), ("R_out", C.c_void_p), ("t_out", C.c_void_p),
                ("inliers_out", C.c_void_p), ("tracked_out", C.c_void_p), ("keyframe_out", C.c_void_p),
                ("n_done", C.c_int), ("rc", C.c_int), ("init_left", C.c_void_p), ("init_right", C.c_void_p),
                ("n_init_points", C.c_int)]


def run_chunks(jobs, pipeline: bool = True, init: bool = False):
    """``svo_vo_run_chunks``: jobs = [(vo, lefts, rights), ...]; front-ends that share a Context run in
    lock step.  With ``init`` every chunk first (re-)initialises on its frame 0 (stereo keyframe,
    identity pose) and tracks frames 1..; outputs then hold ``len(lefts) - 1`` frames.
    Returns one (rc, n_done, R, t, inliers, tracked, keyframe) tuple per job."""
    arr = (_ChunkJob * len(jobs))()
    keep, outs = [], []
    for k, (vo, lefts, rights) in enumerate(jobs):
        if init:
            arr[k].init_left, arr[k].init_right = _ptr(lefts[0]).value, _ptr(rights[0]).value
            lefts, rights = lefts[1:], rights[1:]
        n = len(lefts)
        PtrArr = C.c_void_p * max(n, 1)
        la = PtrArr(*[_ptr(x).value for x in lefts])
        ra = PtrArr(*[_ptr(x).value for x in rights])
        R, t = np.zeros((n, 3, 3)), np.zeros((n, 3))
        inl, trk = np.zeros(n, np.int32), np.zeros(n, np.int32)
        kf = np.zeros(n, np.uint8)
        keep.append((la, ra))
        outs.append((R, t, inl, trk, kf))
        j = arr[k]
        j.vo, j.lefts, j.rights = vo._h, C.addressof(la), C.addressof(ra)
        j.n_frames, j.pipeline = n, int(bool(pipeline))
        j.mem = vo._mem(jobs[k][1][0]) if len(jobs[k][1]) else MEM_DEVICE
        j.R_out, j.t_out, j.inliers_out = _ptr(R), _ptr(t), _ptr(inl)
        j.tracked_out, j.keyframe_out = _ptr(trk), _ptr(kf)
    _check(jobs[0][0].ctx.lib.svo_vo_run_chunks(arr, len(jobs)))
    return [(arr[k].rc, arr[k].n_done, *outs[k][:4], outs[k][4].astype(bool)) for k in range(len(jobs))]


class LcParams(C.Structure):
    _fields_ = [("n_features", C.c_int), ("fast_threshold", C.c_int), ("hamming_threshold", C.c_int),
                ("max_entries", C.c_int), ("use_nss", C.c_int), ("alpha", C.c_float), ("k", C.c_int),
                ("dislocal", C.c_int), ("max_db_results", C.c_int), ("min_nss_factor", C.c_float),
                ("min_matches_per_group", C.c_int), ("max_intragroup_gap", C.c_int),
                ("max_distance_between_groups", C.c_int), ("max_distance_between_queries", C.c_int),
                ("min_Fpoints", C.c_int), ("max_ransac_iterations", C.c_int), ("ransac_probability", C.c_double),
                ("max_reprojection_error", C.c_double), ("max_neighbor_ratio", C.c_double), ("seed", C.c_uint64),
                ("orb_shape", C.c_int), ("orb_levels", C.c_int), ("orb_scale_factor", C.c_float)]


LC_STATUS = ("LOOP_DETECTED", "CLOSE_MATCHES_ONLY", "NO_DB_RESULTS", "LOW_NSS_FACTOR", "LOW_SCORES", "NO_GROUPS",
             "NO_TEMPORAL_CONSISTENCY", "NO_GEOMETRICAL_CONSISTENCY")


class LoopDetector(_Handle):
    """checkLoopDetectorStatus's detector (src/optimizationStuff.cpp:49-64; ``svo_lc``)."""
    _destroy = "svo_lc_destroy"     # waits for the queued work

    def __init__(self, ctx: "Context", w: int, h: int, c: int, **overrides):
        self.ctx = ctx
        self.prm = _make_params(LcParams, "svo_lc_default_params", overrides)
        self._h = C.c_void_p()
        # the images of submitted frames, oldest first: (entry of the submission's last frame, the images) -- the queued work
        # reads them, so each stays referenced until collect / collect_batch / collect_ex has passed that entry
        self._keep_images = collections.deque()
        _check(ctx.lib.svo_lc_create(ctx._h, C.byref(self.prm), w, h, c, C.byref(self._h)))
        ctx._children.add(self)

    @staticmethod
    def _image(image):
        """a host image as the contiguous uint8 array whose pointer is taken; a device image as it is"""
        return np.ascontiguousarray(image, np.uint8) if isinstance(image, np.ndarray) else image

    def _hold(self, images):
        self._keep_images.append((len(self) - 1, images))

    def _release(self):
        """drop the images of every submission whose last frame has been collected"""
        if self._keep_images:
            collected = len(self) - self.pending()
            while self._keep_images and self._keep_images[0][0] < collected:
                self._keep_images.popleft()

    def detect(self, image):
        """-> dict(status, query, match); a detection is status == 0 (LOOP_DETECTED)."""
        image = self._image(image)
        mem = MEM_HOST if isinstance(image, np.ndarray) else MEM_DEVICE
        st, q, m = C.c_int(), C.c_int(), C.c_int()
        _check(self.ctx.lib.svo_lc_detect(self._h, _ptr(image), mem, C.byref(st), C.byref(q), C.byref(m)))
        return dict(status=st.value, query=q.value, match=m.value)

    def submit(self, image):
        """Queue a frame (``svo_lc_submit``): nothing is waited for."""
        image = self._image(image)
        mem = MEM_HOST if isinstance(image, np.ndarray) else MEM_DEVICE
        _check(self.ctx.lib.svo_lc_submit(self._h, _ptr(image), mem))
        self._hold([image])

    def submit_batch(self, images):
        """Queue n frames at once (``svo_lc_submit_batch``): one set of launches per 16 frames."""
        n = len(images)
        if n == 0:
            return
        images = [self._image(im) for im in images]
        mem = MEM_HOST if isinstance(images[0], np.ndarray) else MEM_DEVICE
        ptrs = (C.c_void_p * n)(*[_ptr(im).value for im in images])
        _check(self.ctx.lib.svo_lc_submit_batch(self._h, ptrs, n, mem))
        self._hold(images)

    def collect(self):
        """The verdict of the oldest queued frame (``svo_lc_collect``) -> dict(status, query, match)."""
        st, q, m = C.c_int(), C.c_int(), C.c_int()
        _check(self.ctx.lib.svo_lc_collect(self._h, C.byref(st), C.byref(q), C.byref(m)))
        self._release()
        return dict(status=st.value, query=q.value, match=m.value)

    def collect_batch(self, n: int):
        """``svo_lc_collect_batch``: the verdicts of the n oldest queued frames in one call -> list of dict(status, query, match)."""
        n = int(n)
        st, q, m = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(self.ctx.lib.svo_lc_collect_batch(self._h, n, _ptr(st), _ptr(q), _ptr(m)))
        self._release()
        return [dict(status=a, query=b, match=c) for a, b, c in zip(st.tolist(), q.tolist(), m.tolist())]

    def pending(self) -> int:
        return self.ctx.lib.svo_lc_pending(self._h)

    def set_vocabulary(self, voc: "Vocabulary", di_levels: int = 2):
        """DBoW2's scoring and the direct-index geometric check (``svo_lc_set_vocabulary``); before the first frame."""
        _check(self.ctx.lib.svo_lc_set_vocabulary(self._h, voc._h, int(di_levels)))
        self._voc = voc      # the vocabulary must outlive the detector

    def submit_features(self, xy, desc):
        """Queue a frame given by its features (``svo_lc_submit_features``): xy [n, 2] float32, desc [n, 8] uint32."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        desc = np.ascontiguousarray(desc, np.uint32).reshape(-1, 8)
        _check(self.ctx.lib.svo_lc_submit_features(self._h, _ptr(xy), _ptr(desc), len(xy), MEM_HOST))

    def submit_features_batch(self, n, xy, desc):
        """``svo_lc_submit_features_batch``: n [F] int32, xy [F, cap, 2] float32, desc [F, cap, 8] uint32 (host arrays)."""
        n = np.ascontiguousarray(n, np.int32)
        xy = np.ascontiguousarray(xy, np.float32)
        desc = np.ascontiguousarray(desc, np.uint32)
        assert xy.shape[0] == len(n) == desc.shape[0] and xy.shape[1] == desc.shape[1]
        _check(self.ctx.lib.svo_lc_submit_features_batch(self._h, _ptr(xy), _ptr(desc), _ptr(n), len(n), xy.shape[1], MEM_HOST))

    def fill_features_batch(self, n, xy, desc):
        """``svo_lc_fill_features_batch``: database entries that are not queries (arrays as :meth:`submit_features_batch`)."""
        n = np.ascontiguousarray(n, np.int32)
        xy = np.ascontiguousarray(xy, np.float32)
        desc = np.ascontiguousarray(desc, np.uint32)
        assert xy.shape[0] == len(n) == desc.shape[0] and xy.shape[1] == desc.shape[1]
        if len(n):
            _check(self.ctx.lib.svo_lc_fill_features_batch(self._h, _ptr(xy), _ptr(desc), _ptr(n), len(n), xy.shape[1], MEM_HOST))

    def collect_ex(self):
        """``svo_lc_collect_ex`` -> dict(status, query, match, cand_id, cand_score, ns_factor)."""
        st, q, m, n, ns = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_double()
        ids, sc = np.zeros(64, np.int32), np.zeros(64)
        _check(self.ctx.lib.svo_lc_collect_ex(self._h, C.byref(st), C.byref(q), C.byref(m), _ptr(ids), _ptr(sc), 64,
                                              C.byref(n), C.byref(ns)))
        self._release()
        k = min(n.value, 64)
        return dict(status=st.value, query=q.value, match=m.value, cand_id=ids[:k].copy(), cand_score=sc[:k].copy(),
                    ns_factor=ns.value)

    def __len__(self):
        return self.ctx.lib.svo_lc_size(self._h)

    def close(self):
        super().close()
        self._keep_images.clear()


class Vocabulary(_Handle):
    """DBoW2's OrbVocabulary on the GPU (``svo_voc``): ``train`` (src/bagOfWordsDetector.cpp:46-56) or ``from_arrays``
    (a vocabulary read from a file, ros_stereo_slam_amd/vocabulary.py)."""
    _destroy = "svo_voc_destroy"

    def __init__(self, ctx: "Context", handle):
        self.ctx, self._h = ctx, handle
        k, L, nn, nw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _check(ctx.lib.svo_voc_info(handle, C.byref(k), C.byref(L), C.byref(nn), C.byref(nw)))
        self.k, self.L, self.n_nodes, self.n_words = k.value, L.value, nn.value, nw.value
        ctx._children.add(self)

    @classmethod
    def train(cls, ctx: "Context", descs_per_image, k=9, L=6, seed=0):
        off = np.zeros(len(descs_per_image) + 1, np.int32)
        off[1:] = np.cumsum([len(d) for d in descs_per_image])
        D = np.ascontiguousarray(np.concatenate([np.asarray(d, np.uint32).reshape(-1, 8) for d in descs_per_image]), np.uint32)
        h = C.c_void_p()
        _check(ctx.lib.svo_voc_train(ctx._h, _ptr(D), _ptr(off), len(descs_per_image), int(k), int(L), C.c_uint64(seed),
                                     C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_arrays(cls, ctx: "Context", k, L, parent, desc, weight):
        parent = np.ascontiguousarray(parent, np.int32)
        desc = np.ascontiguousarray(desc, np.uint32).reshape(-1, 8)
        weight = np.ascontiguousarray(weight, np.float64)
        h = C.c_void_p()
        _check(ctx.lib.svo_voc_create(ctx._h, int(k), int(L), len(parent), _ptr(parent), _ptr(desc), _ptr(weight), C.byref(h)))
        return cls(ctx, h)

    def arrays(self):
        n = self.n_nodes
        out = dict(parent=np.zeros(n, np.int32), desc=np.zeros((n, 8), np.uint32), weight=np.zeros(n),
                   word_id=np.zeros(n, np.int32))
        _check(self.ctx.lib.svo_voc_export(self._h, _ptr(out["parent"]), _ptr(out["desc"]), _ptr(out["weight"]),
                                           _ptr(out["word_id"])))
        return out

    def transform(self, desc, levelsup=0):
        desc = np.ascontiguousarray(desc, np.uint32).reshape(-1, 8)
        n = len(desc)
        word, node, weight = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1))
        _check(self.ctx.lib.svo_voc_transform(self._h, _ptr(desc), n, int(levelsup), _ptr(word), _ptr(weight), _ptr(node),
                                              MEM_HOST))
        return word[:n], weight[:n], node[:n]

    def bow(self, desc, levelsup=0):
        """-> (words ascending, values L1-normalised, direct-index node per feature, -1 = not indexed)"""
        desc = np.ascontiguousarray(desc, np.uint32).reshape(-1, 8)
        n = len(desc)
        w, v, node, m = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1)), np.zeros(max(n, 1), np.int32), C.c_int()
        _check(self.ctx.lib.svo_voc_bow(self._h, _ptr(desc), n, int(levelsup), _ptr(w), _ptr(v), C.byref(m), _ptr(node)))
        return w[:m.value].copy(), v[:m.value].copy(), node[:n].copy()


class KeyframeMap(_Handle):
    """keyFrameHistory / mapHistory in HBM and visualSLAM::updateOdometry on it
    (src/optimizationStuff.cpp:17-47; ``svo_map``)."""
    _destroy = "svo_map_destroy"

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self._h = C.c_void_p()
        _check(ctx.lib.svo_map_create(ctx._h, C.byref(self._h)))
        ctx._children.add(self)

    def add_keyframe(self, traj_index: int, R, t, xyz_cam, retrack: bool = True, n: int | None = None):
        """xyz_cam: numpy (n, 3) float32 or a device pointer / tensor with ``n`` given."""
        if isinstance(xyz_cam, np.ndarray):
            xyz_cam = np.ascontiguousarray(xyz_cam, np.float32).reshape(-1, 3)
            n, mem = xyz_cam.shape[0], MEM_HOST
        else:
            mem = MEM_DEVICE
        _check(self.ctx.lib.svo_map_add_keyframe(self._h, int(traj_index), _ptr(np.ascontiguousarray(R, np.float64)),
                                                 _ptr(np.ascontiguousarray(t, np.float64)), _ptr(xyz_cam), int(n),
                                                 int(bool(retrack)), mem))

    def add_from_vo(self, vo: "VisualOdometry", traj_index: int, R, t, retrack: bool = True):
        """The front-end's last keyframe cloud, device to device (no host copy)."""
        import torch

        n = C.c_int()
        _check(self.ctx.lib.svo_vo_get_keyframe_cloud(vo._h, None, 0, C.byref(n), MEM_DEVICE))
        buf = torch.empty((max(n.value, 1), 3), dtype=torch.float32, device="cuda")
        _check(self.ctx.lib.svo_vo_get_keyframe_cloud(vo._h, _ptr(buf), n.value, C.byref(n), MEM_DEVICE))
        self.add_keyframe(traj_index, R, t, buf, retrack, n=n.value)
        self.ctx.sync()  # buf goes out of scope
        return n.value

    def update(self, translations):
        t = np.ascontiguousarray(translations, np.float64).reshape(-1, 3)
        _check(self.ctx.lib.svo_map_update(self._h, _ptr(t), t.shape[0]))

    def __len__(self):
        return self.ctx.lib.svo_map_num_keyframes(self._h)

    def points(self):
        """-> (xyz_world (N, 3) float32, counts per retrack keyframe)."""
        npts, nkf = C.c_size_t(), C.c_int()
        _check(self.ctx.lib.svo_map_get_points(self._h, None, C.c_size_t(0), None, 0, C.byref(npts), C.byref(nkf), MEM_HOST))
        xyz = np.zeros((max(npts.value, 1), 3), np.float32)
        counts = np.zeros(max(nkf.value, 1), np.int32)
        _check(self.ctx.lib.svo_map_get_points(self._h, _ptr(xyz), C.c_size_t(npts.value), _ptr(counts), nkf.value,
                                               C.byref(npts), C.byref(nkf), MEM_HOST))
        return xyz[:npts.value], counts[:nkf.value]


INFO_TRIU = np.triu_indices(6)


def _info21(info):
    """None, 21 numbers or a 6 x 6 matrix -> None or a contiguous float64 [21] (upper triangle, row-major)"""
    if info is None:
        return None
    a = np.asarray(info, np.float64)
    if a.shape == (6, 6):
        a = a[INFO_TRIU]
    return np.ascontiguousarray(a, np.float64).reshape(21)


def info_matrix(info21) -> np.ndarray:
    """The symmetric 6 x 6 matrix of 21 upper-triangle numbers"""
    M = np.zeros((6, 6))
    M[INFO_TRIU] = np.asarray(info21, np.float64).reshape(21)
    return M + np.triu(M, 1).T


class ClosureParams(C.Structure):
    _fields_ = [("f_thr", C.c_double), ("pnp_iterations", C.c_int), ("pnp_reproj_err", C.c_double),
                ("pnp_confidence", C.c_double), ("seed", C.c_uint64)]


def closure_params(**overrides) -> ClosureParams:
    _known_fields(ClosureParams, "svo_closure_params", overrides)
    return _make_params(ClosureParams, "svo_closure_default_params", overrides)


@_ctx_method
def measure_closure(self, newest, matched, xy, xyz, K4, size=None, **params):
    """getLCMeasurement (``svo_closure_measure``): the relative pose X_newest^-1 X_matched from the newest frame's image, its
    points ``xy`` [n, 2] and their 3-D positions ``xyz`` [n, 3] in that camera's frame, and the matched frame's image.
    Host arrays (images [h, w, c] uint8), or device tensors / addresses with ``size=(w, h, c, n)``.
    -> (rc, meas7 or None, n_tracked, n_inliers); rc is SVO_OK or SVO_ERR_TRACKING_LOST (fewer than 6 PnP inliers)."""
    prm = closure_params(**params)
    if size is None:
        newest = np.ascontiguousarray(newest, np.uint8)
        matched = np.ascontiguousarray(matched, np.uint8)
        if newest.ndim == 2:
            newest, matched = newest[:, :, None], matched[:, :, None]
        assert newest.shape == matched.shape
        h, w, c = newest.shape
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        assert len(xy) == len(xyz)
        n, mem = len(xy), MEM_HOST
    else:
        (w, h, c, n), mem = size, MEM_DEVICE
    K = np.ascontiguousarray(K4, np.float64).reshape(4)
    meas = np.zeros(7)
    ntrk, ninl = C.c_int(), C.c_int()
    rc = self.lib.svo_closure_measure(self._h, _ptr(newest), _ptr(matched), int(w), int(h), int(c), _ptr(xy), _ptr(xyz), int(n),
                                      _ptr(K), C.byref(prm), _ptr(meas), C.byref(ntrk), C.byref(ninl), mem)
    if rc not in (SVO_OK, SVO_ERR_TRACKING_LOST):
        _check(rc)
    return rc, (meas if rc == SVO_OK else None), ntrk.value, ninl.value


class PoseGraph(_Handle):
    """SE3 pose graph on the GPU (``svo_posegraph``), mirroring globalPoseGraph
    (include/poseGraph.h:36-179).  Poses: tx ty tz qx qy qz qw."""
    _destroy = "svo_pg_destroy"

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._h = C.c_void_p()
        _check(ctx.lib.svo_pg_create(ctx._h, C.byref(self._h)))
        ctx._children.add(self)

    def augment_node(self, pose7):
        _check(self.ctx.lib.svo_pg_augment_node(self._h, _ptr(np.ascontiguousarray(pose7, np.float64))))

    def add_loop_closure(self, from_id: int, meas7=None, info21=None):
        """Edge (previous vertex -> from_id).  Without arguments: the reference's identity closure
        (``svo_pg_add_loop_closure``).  ``meas7``: the measured relative pose (tx ty tz qx qy qz qw, e.g. from
        ``measure_closure``); ``info21``: the upper triangle of the 6 x 6 information matrix, row-major, or the matrix."""
        if meas7 is None and info21 is None:
            _check(self.ctx.lib.svo_pg_add_loop_closure(self._h, int(from_id)))
            return
        z = None if meas7 is None else np.ascontiguousarray(meas7, np.float64).reshape(7)
        om = _info21(info21)   # z / om stay referenced until the call has returned
        _check(self.ctx.lib.svo_pg_add_loop_closure_measured(self._h, int(from_id), _ptr(z), _ptr(om)))

    def set_edge_information(self, e: int, info21):
        """``svo_pg_set_edge_information``: 21 numbers (upper triangle, row-major), a 6 x 6 matrix, or None = identity."""
        om = _info21(info21)
        _check(self.ctx.lib.svo_pg_set_edge_information(self._h, int(e), _ptr(om)))

    def edge_information(self, e: int) -> np.ndarray:
        """The 21 numbers of edge e's information matrix (the identity's when none is stored)."""
        out = np.zeros(21)
        _check(self.ctx.lib.svo_pg_get_edge_information(self._h, int(e), _ptr(out)))
        return out

    def set_robust_kernel(self, e: int, kind: int, delta: float = 0.0):
        """``svo_pg_set_robust_kernel``: kind = PG_ROBUST_NONE / HUBER / CAUCHY / DCS / GEMAN_MCCLURE and its parameter."""
        _check(self.ctx.lib.svo_pg_set_robust_kernel(self._h, int(e), int(kind), C.c_double(delta)))

    def robust_kernel(self, e: int):
        """-> (kind, delta) of edge e; (PG_ROBUST_NONE, 0.0) when it carries none."""
        kind, delta = C.c_int(), C.c_double()
        _check(self.ctx.lib.svo_pg_get_robust_kernel(self._h, int(e), C.byref(kind), C.byref(delta)))
        return kind.value, delta.value

    def set_loop_closure_kernel(self, kind: int, delta: float = 0.0):
        """``svo_pg_set_loop_closure_kernel``: the kernel of every loop closure added from now on."""
        _check(self.ctx.lib.svo_pg_set_loop_closure_kernel(self._h, int(kind), C.c_double(delta)))

    def edge_residuals(self):
        """``svo_pg_edge_residuals`` -> (chi2, weight, rho), one double per edge, at the current estimates."""
        out = np.zeros((3, self.num_edges))
        _check(self.ctx.lib.svo_pg_edge_residuals(self._h, _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return out[0], out[1], out[2]

    def linearization_weights(self) -> np.ndarray:
        """``svo_pg_linearization_weights``: the weights the last optimize's final linearisation stored."""
        out = np.zeros(self.num_edges)
        _check(self.ctx.lib.svo_pg_linearization_weights(self._h, _ptr(out)))
        return out

    def prune_edges(self, threshold: float = 0.25, cap: int | None = None) -> np.ndarray:
        """``svo_pg_prune_edges`` -> the former indices of the removed edges, ascending (cap: slots offered, default every edge)."""
        cap = self.num_edges if cap is None else int(cap)
        removed, n = np.zeros(max(cap, 1), np.int32), C.c_int()
        _check(self.ctx.lib.svo_pg_prune_edges(self._h, C.c_double(threshold), _ptr(removed), cap, C.byref(n)))
        return removed[:n.value].copy()

    def augment_nodes(self, poses7, closure_from=None):
        """``svo_pg_augment_nodes``: poses7 [n, 7]; closure_from [n] int32 (-1: none): the closure edge staged before node i."""
        p = np.ascontiguousarray(poses7, np.float64).reshape(-1, 7)
        cf = None if closure_from is None else np.ascontiguousarray(closure_from, np.int32)
        assert cf is None or len(cf) == len(p)
        _check(self.ctx.lib.svo_pg_augment_nodes(self._h, len(p), _ptr(p), _ptr(cf)))

    def optimize(self, iters: int = 10) -> np.ndarray:
        chi2 = np.zeros(iters + 1)
        _check(self.ctx.lib.svo_pg_optimize(self._h, iters, _ptr(chi2)))
        return chi2

    @property
    def num_vertices(self) -> int:
        return self.ctx.lib.svo_pg_num_vertices(self._h)

    @property
    def num_edges(self) -> int:
        return self.ctx.lib.svo_pg_num_edges(self._h)

    def set_refinement(self, passes: int):
        """``svo_pg_set_refinement``: iterative-refinement passes per Gauss-Newton step (0 = g2o's single solve)."""
        _check(self.ctx.lib.svo_pg_set_refinement(self._h, int(passes)))

    def estimates(self) -> np.ndarray:
        out = np.zeros((self.num_vertices, 7))
        _check(self.ctx.lib.svo_pg_get_estimates(self._h, _ptr(out)))
        return out

    def edges(self):
        res = []
        for e in range(self.num_edges):
            a, b, z = C.c_int(), C.c_int(), np.zeros(7)
            _check(self.ctx.lib.svo_pg_get_edge(self._h, e, C.byref(a), C.byref(b), _ptr(z)))
            res.append((a.value, b.value, z))
        return res

    def read_g2o(self, path, information: bool = False):
        """information=True keeps the information matrices of the EDGE_SE3:QUAT lines (``svo_pg_read_g2o_info``)."""
        fn = self.ctx.lib.svo_pg_read_g2o_info if information else self.ctx.lib.svo_pg_read_g2o
        _check(fn(self._h, os.fspath(path).encode()))

    def write_g2o(self, path):
        _check(self.ctx.lib.svo_pg_write_g2o(self._h, os.fspath(path).encode()))


# ---- point-to-plane ICP between clouds and the information of the edge it yields (csrc/cloud.hip) ------------------
class IcpParams(C.Structure):
    _fields_ = [("max_iteration", C.c_int), ("relative_fitness", C.c_double), ("relative_rmse", C.c_double)]


def icp_params(**overrides) -> IcpParams:
    _known_fields(IcpParams, "svo_icp_params", overrides)
    return _make_params(IcpParams, "svo_icp_default_params", overrides)


def _cloud_arg(xyz):
    """numpy array or device tensor (float32, n x 3) -> (array, n, mem)"""
    if _is_device(xyz):
        import torch

        t = xyz.reshape(-1, 3).contiguous()
        assert t.dtype == torch.float32
        torch.cuda.synchronize(t.device)
        return t, int(t.shape[0]), MEM_DEVICE
    a = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    return a, int(a.shape[0]), MEM_HOST


def _T16(T):
    return np.ascontiguousarray(np.eye(4) if T is None else T, np.float64).reshape(16)


class Cloud(_Handle):
    """A resident target cloud with its search index (``svo_cloud``): n x 3 float32 points, host array or device tensor."""
    _destroy = "svo_cloud_destroy"

    def __init__(self, ctx: Context, xyz):
        self.ctx = ctx
        self._h = C.c_void_p()
        a, n, mem = _cloud_arg(xyz)
        _check(ctx.lib.svo_cloud_create(ctx._h, _ptr(a), n, mem, C.byref(self._h)))
        ctx._children.add(self)

    def __len__(self) -> int:
        return self.ctx.lib.svo_cloud_size(self._h)

    @property
    def has_normals(self) -> bool:
        return bool(self.ctx.lib.svo_cloud_has_normals(self._h))

    def set_normals(self, normals):
        a = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
        assert len(a) == len(self)
        _check(self.ctx.lib.svo_cloud_set_normals(self._h, _ptr(a), MEM_HOST))

    def normals(self) -> np.ndarray:
        out = np.zeros((len(self), 3))
        _check(self.ctx.lib.svo_cloud_get_normals(self._h, _ptr(out), MEM_HOST))
        return out

    def knn(self, k: int = 30) -> np.ndarray:
        """[n, k] int32: the k nearest points of every point, itself included, by (d2, index); -1 past a short list"""
        out = np.zeros((len(self), max(int(k), 1)), np.int32)
        _check(self.ctx.lib.svo_cloud_knn(self._h, int(k), _ptr(out), MEM_HOST))
        return out

    def estimate_normals(self, knn: int = 30):
        _check(self.ctx.lib.svo_cloud_estimate_normals(self._h, int(knn)))
        return self


@_ctx_method
def icp_correspondences(self, src, target: Cloud, max_dist, T=None):
    """``svo_icp_correspondences`` -> (corr [n_src] int32, fitness, rmse)"""
    a, n, mem = _cloud_arg(src)
    if mem == MEM_DEVICE:
        import torch

        corr = torch.empty(max(n, 1), dtype=torch.int32, device=a.device)
    else:
        corr = np.zeros(max(n, 1), np.int32)
    fit, rmse = C.c_double(), C.c_double()
    _check(self.lib.svo_icp_correspondences(self._h, _ptr(a), n, target._h, C.c_double(max_dist), _ptr(_T16(T)), _ptr(corr),
                                            C.byref(fit), C.byref(rmse), mem))
    return corr[:n], fit.value, rmse.value


@_ctx_method
def icp_normal_equations(self, src, target: Cloud, max_dist, T=None):
    """``svo_icp_normal_equations``: one point-to-plane step at T -> (JtJ21, Jtr6, n_corr)"""
    a, n, mem = _cloud_arg(src)
    A, b, nc = np.zeros(21), np.zeros(6), C.c_int()
    _check(self.lib.svo_icp_normal_equations(self._h, _ptr(a), n, target._h, C.c_double(max_dist), _ptr(_T16(T)), _ptr(A),
                                             _ptr(b), C.byref(nc), mem))
    return A, b, nc.value


@_ctx_method
def icp_point_to_plane(self, src, target: Cloud, max_dist, T_init=None, want_corr=False, **params):
    """``svo_icp_point_to_plane`` -> (T [4, 4], fitness, rmse, iterations[, corr])"""
    a, n, mem = _cloud_arg(src)
    prm = icp_params(**params)
    T, fit, rmse, its = np.zeros(16), C.c_double(), C.c_double(), C.c_int()
    corr = None
    if want_corr:
        if mem == MEM_DEVICE:
            import torch

            corr = torch.empty(max(n, 1), dtype=torch.int32, device=a.device)
        else:
            corr = np.zeros(max(n, 1), np.int32)
    _check(self.lib.svo_icp_point_to_plane(self._h, _ptr(a), n, target._h, C.c_double(max_dist), _ptr(_T16(T_init)),
                                           C.byref(prm), _ptr(T), C.byref(fit), C.byref(rmse), C.byref(its), _ptr(corr), mem))
    res = (T.reshape(4, 4), fit.value, rmse.value, its.value)
    return res + (corr[:n],) if want_corr else res


@_ctx_method
def icp_information(self, src, target: Cloud, max_dist, T=None):
    """``svo_icp_information`` -> (Lambda [6, 6], n_corr)"""
    a, n, mem = _cloud_arg(src)
    L, nc = np.zeros(36), C.c_int()
    _check(self.lib.svo_icp_information(self._h, _ptr(a), n, target._h, C.c_double(max_dist), _ptr(_T16(T)), _ptr(L),
                                        C.byref(nc), mem))
    return L.reshape(6, 6), nc.value


@_ctx_method
def icp_pairwise(self, src, target: Cloud, dist_coarse=15.0, dist_fine=1.5, **params):
    """``svo_icp_pairwise`` (pairwiseRegistration) -> (T [4, 4], Lambda [6, 6], details); details: fitness / rmse /
    iterations of the coarse and the fine pass, n_corr of the information"""
    a, n, mem = _cloud_arg(src)
    prm = icp_params(**params)
    T, L, fit, rmse, its, nc = np.zeros(16), np.zeros(36), np.zeros(2), np.zeros(2), np.zeros(2, np.int32), C.c_int()
    _check(self.lib.svo_icp_pairwise(self._h, _ptr(a), n, target._h, C.c_double(dist_coarse), C.c_double(dist_fine),
                                     C.byref(prm), _ptr(T), _ptr(L), _ptr(fit), _ptr(rmse), _ptr(its), C.byref(nc), mem))
    return T.reshape(4, 4), L.reshape(6, 6), dict(fitness=fit, rmse=rmse, iterations=its, n_corr=nc.value)


def icp_edge_information(info, T) -> np.ndarray:
    """``svo_icp_edge_information``: Lambda [6, 6] of a registration with result T -> the 21 numbers
    ``PoseGraph.add_loop_closure`` / ``set_edge_information`` take for an edge whose measurement is T"""
    L = np.ascontiguousarray(info, np.float64).reshape(36)
    out = np.zeros(21)
    _check(load().svo_icp_edge_information(_ptr(L), _ptr(_T16(T)), _ptr(out)))
    return out


def icp_meas7(T) -> np.ndarray:
    """``svo_icp_meas7``: T [4, 4] -> tx ty tz qx qy qz qw (w >= 0)"""
    out = np.zeros(7)
    _check(load().svo_icp_meas7(_ptr(_T16(T)), _ptr(out)))
    return out
