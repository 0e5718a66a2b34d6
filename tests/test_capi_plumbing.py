"""The plumbing ros_stereo_slam_amd/capi.py shares (CPU only): the column layout of the batched detectors against the byte offsets
the wrappers used to spell out as literals, the parameter makers against the library's own defaults, and the handle base's
close() / __del__ around a fake destroy function.  tests/test_gpu_capi_batch.py runs the wrappers built on them."""
import ctypes as C
import pathlib
import re
import types

import numpy as np
import pytest

from ros_stereo_slam_amd import capi

F32, I32 = np.float32, np.int32


def load_library():
    """torch ships its own HIP runtime: let it load first, as the ctx fixture of tests/conftest.py does, so that one copy serves torch
    and libsvo_hip whichever test of a session comes first."""
    import torch

    torch.cuda.is_available()
    return capi.load()


# ---- layout: the literals of the wrappers before they shared _column_layout, in units of e = nimg * cap bytes ----------------------
#   spec -> ({column: (buffer, offset / e)}, float buffer bytes / e, int buffer bytes / e)
LITERALS = {
    "sift": (capi._SIFT_COLUMNS, {"xy": (F32, 0), "size": (F32, 8), "angle": (F32, 12), "response": (F32, 16), "octave": (I32, 0),
                                  "desc": (F32, 20)}, 4 * (5 + 128), 4),
    "sift without descriptors": (capi._SIFT_COLUMNS[:-1], {"xy": (F32, 0), "size": (F32, 8), "angle": (F32, 12), "response": (F32, 16),
                                                           "octave": (I32, 0)}, 4 * 5, 4),
    "surf": (capi._SURF_COLUMNS, {"xy": (F32, 0), "size": (F32, 8), "angle": (F32, 12), "response": (F32, 16), "octave": (I32, 0),
                                  "laplacian": (I32, 4), "desc": (F32, 20)}, 4 * (5 + 64), 8),
    "surf without descriptors": (capi._SURF_COLUMNS[:-1], {"xy": (F32, 0), "size": (F32, 8), "angle": (F32, 12), "response": (F32, 16),
                                                           "octave": (I32, 0), "laplacian": (I32, 4)}, 4 * 5, 8),
    "fast": (capi._FAST_COLUMNS, {"xy": (F32, 0), "response": (F32, 8)}, 12, 0),
    "star": (capi._STAR_COLUMNS, {"xy": (F32, 0), "size": (F32, 8), "response": (F32, 12)}, 16, 0),
}


@pytest.mark.parametrize("e", [1, 7, 16 * 20000])
@pytest.mark.parametrize("name", sorted(LITERALS))
def test_column_layout_is_the_literals(name, e):
    spec, where, fbytes, ibytes = LITERALS[name]
    cols, got_f, got_i = capi._column_layout(spec, e)
    assert list(cols) == [c[0] for c in spec] == list(where)          # the order of the entry point's arguments
    assert {k: (dt, off) for k, (dt, off, _) in cols.items()} == {k: (dt, off * e) for k, (dt, off) in where.items()}
    assert (got_f, got_i) == (fbytes * e, ibytes * e)
    # the columns of a buffer tile it: no overlap, no gap
    for dt, total in ((F32, got_f), (I32, got_i)):
        spans = sorted((off, off + 4 * e * width) for d, off, width in cols.values() if d is dt)
        assert [a for a, _ in spans] == [0, *(b for _, b in spans)][:len(spans)] and (spans[-1][1] if spans else 0) == total


def test_column_widths_are_the_outputs():
    assert {c[0]: c[2] for c in capi._SIFT_COLUMNS} == dict(xy=2, size=1, angle=1, response=1, octave=1, desc=128)
    assert {c[0]: c[2] for c in capi._SURF_COLUMNS} == dict(xy=2, size=1, angle=1, response=1, octave=1, laplacian=1, desc=64)
    assert {c[0]: c[2] for c in capi._FAST_COLUMNS} == dict(xy=2, response=1)
    assert {c[0]: c[2] for c in capi._STAR_COLUMNS} == dict(xy=2, size=1, response=1)


# ---- params ------------------------------------------------------------------------------------------------------------------------
#   maker, struct, the library's default function, an override, what an unknown field raises
PARAMS = {
    "orb": (capi.orb_params, capi.OrbParams, "svo_orb_default_params", ("n_features", 123), AssertionError),
    "sgbm": (capi.sgbm_params, capi.SgbmParams, "svo_sgbm_default_params", ("p2", 777), AssertionError),
    "sift": (capi.sift_params, capi.SiftParams, "svo_sift_default_params", ("sigma", 1.25), AssertionError),
    "fast": (capi.fast_params, capi.FastParams, "svo_fast_default_params", ("max_keypoints", 9), AssertionError),
    "star": (capi.star_params, capi.StarParams, "svo_star_default_params", ("response_threshold", 11), AssertionError),
    "surf": (capi.surf_params, capi.SurfParams, "svo_surf_default_params", ("n_octaves", 2), AssertionError),
    "wls": (capi.wls_params, capi.WlsParams, "svo_wls_default_params", ("sigma_color", 2.5), AssertionError),
    # these three have always refused an unknown field with a TypeError that names the struct and the field
    "closure": (capi.closure_params, capi.ClosureParams, "svo_closure_default_params", ("pnp_iterations", 17), TypeError),
    "icp": (capi.icp_params, capi.IcpParams, "svo_icp_default_params", ("max_iteration", 3), TypeError),
    "ba_window": (capi.ba_window_params.default, capi.ba_window_params, "svo_ba_window_default_params", ("iterations", 3), TypeError),
}


def fields(p):
    return {n: getattr(p, n) for n, _ in p._fields_}


def library_defaults(name):
    _, cls, fn, _, _ = PARAMS[name]
    p = cls()
    before = (C.byref(library_defaults("sgbm")),) if name == "wls" else ()
    getattr(load_library(), fn)(*before, C.byref(p))
    return p


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_params_maker(name):
    maker, cls, _, (field, value), unknown = PARAMS[name]
    want = fields(library_defaults(name))
    p = maker()
    assert type(p) is cls and fields(p) == want
    assert want[field] != value
    assert fields(maker(**{field: value})) == {**want, field: value}
    with pytest.raises(unknown, match="no_such_field"):
        maker(no_such_field=1)
    with pytest.raises(unknown, match="no_such_field"):
        maker(**{field: value, "no_such_field": 1})


def test_make_params_asserts_on_an_unknown_field():
    p = capi._make_params(capi.FastParams, "svo_fast_default_params", dict(threshold=3))
    assert fields(p) == {**fields(library_defaults("fast")), "threshold": 3}
    with pytest.raises(AssertionError, match="^nope$"):
        capi._make_params(capi.FastParams, "svo_fast_default_params", dict(threshold=3, nope=1))


def test_wls_params_follow_the_left_matcher():
    left = capi.sgbm_params(min_disparity=8, num_disparities=64)
    want = capi.WlsParams()
    load_library().svo_wls_default_params(C.byref(left), C.byref(want))
    assert fields(capi.wls_params(left)) == fields(want) != fields(capi.wls_params())
    assert fields(capi.wls_params(left, lrc_thresh=5)) == {**fields(want), "lrc_thresh": 5}
    right = capi.SgbmParams()
    load_library().svo_sgbm_right_matcher_params(C.byref(left), C.byref(right))
    assert fields(capi.sgbm_right_params(left)) == fields(right)


@pytest.mark.parametrize("name, helper", [("sift", capi._sift_prm), ("surf", capi._surf_prm), ("star", capi._star_prm),
                                          ("wls", lambda v: capi._wls_prm(None, v))])
def test_struct_or_dict_or_none(name, helper):
    maker, cls, _, (field, value), unknown = PARAMS[name]
    p = maker(**{field: value})
    assert helper(p) is p and capi._as_params(cls, maker, p) is p
    assert fields(helper(None)) == fields(maker())
    assert fields(helper({})) == fields(maker())
    assert fields(helper({field: value})) == fields(p)
    with pytest.raises(unknown, match="no_such_field"):
        helper({"no_such_field": 1})


def test_wls_prm_takes_its_defaults_from_the_matcher_given():
    left = capi.sgbm_params(min_disparity=8, num_disparities=64)
    assert fields(capi._wls_prm(left, {"lrc_thresh": 5})) == fields(capi.wls_params(left, lrc_thresh=5))
    assert fields(capi._wls_prm(left, None)) == fields(capi.wls_params(left))


# ---- the handle base ---------------------------------------------------------------------------------------------------------------
def fake_handle(takes_ctx, destroy):
    """A _Handle subclass instance around ``destroy``, a context stand-in that holds handle 7, and no library"""
    ctx = types.SimpleNamespace(lib=types.SimpleNamespace(fake_destroy=destroy), _h=C.c_void_p(7))
    cls = type("Fake", (capi._Handle,), dict(_destroy="fake_destroy", _destroy_takes_ctx=takes_ctx))
    obj = cls()
    obj.ctx, obj._h = ctx, C.c_void_p(5)
    return obj, ctx


@pytest.mark.parametrize("takes_ctx", [True, False])
def test_close_destroys_once(takes_ctx):
    calls = []
    obj, ctx = fake_handle(takes_ctx, lambda *a: calls.append(tuple(x.value for x in a)))
    obj.close()
    assert calls == [(7, 5) if takes_ctx else (5,)] and not obj._h
    obj.close()
    obj.__del__()
    assert len(calls) == 1


def test_close_after_the_context_is_gone_destroys_nothing():
    calls = []
    obj, ctx = fake_handle(True, lambda *a: calls.append(a))
    ctx._h = C.c_void_p()
    obj.close()
    assert calls == [] and not obj._h


def test_del_swallows_what_destroy_raises():
    def destroy(*a):
        raise RuntimeError("destroy failed")

    obj, _ = fake_handle(False, destroy)
    with pytest.raises(RuntimeError):
        obj.close()
    obj.__del__()
    del obj


def test_every_owned_class_names_its_destroy_function():
    owned = {capi.Pyramid: ("svo_pyramid_destroy", True), capi.RectifyMap: ("svo_rectify_map_destroy", True),
             capi.VisualOdometry: ("svo_vo_destroy", False), capi.LoopDetector: ("svo_lc_destroy", False),
             capi.Vocabulary: ("svo_voc_destroy", False), capi.KeyframeMap: ("svo_map_destroy", False),
             capi.PoseGraph: ("svo_pg_destroy", False), capi.Cloud: ("svo_cloud_destroy", False)}
    lib = load_library()
    for cls, (name, takes_ctx) in owned.items():
        assert issubclass(cls, capi._Handle) and (cls._destroy, cls._destroy_takes_ctx) == (name, takes_ctx)
        assert name in capi.declared_symbols() and hasattr(lib, name)
        assert "close" not in vars(cls) or cls is capi.LoopDetector
        assert "__del__" not in vars(cls)
    # the context closes its children itself, and the communicator is no child of it
    assert not issubclass(capi.Context, capi._Handle) and not issubclass(capi.ShardComm, capi._Handle)


def test_loop_detector_close_drops_the_held_images():
    calls = []
    det = capi.LoopDetector.__new__(capi.LoopDetector)
    det.ctx = types.SimpleNamespace(lib=types.SimpleNamespace(svo_lc_destroy=lambda h: calls.append(h.value)), _h=C.c_void_p(7))
    det._h, det._keep_images = C.c_void_p(5), capi.collections.deque([(0, ["image"])])
    det.close()
    assert calls == [5] and not det._h and not det._keep_images


# ---- small things ------------------------------------------------------------------------------------------------------------------
def test_mem_of_and_image_shape():
    assert capi._mem_of(True) == capi.MEM_DEVICE and capi._mem_of(False) == capi.MEM_HOST
    assert capi._image_shape(np.zeros((3, 5), np.uint8)) == (5, 3, 1)
    assert capi._image_shape(np.zeros((3, 5, 3), np.uint8)) == (5, 3, 3)


def test_cut_copies_each_image_s_rows():
    a, b = np.arange(24, dtype=F32).reshape(2, 6, 2), np.arange(12, dtype=I32).reshape(2, 6)
    out = capi._cut([a, None, b], [2, 0])
    assert [len(o) for o in out] == [3, 3] and out[0][1] is None and out[1][1] is None
    assert np.array_equal(out[0][0], a[0, :2]) and np.array_equal(out[0][2], b[0, :2])
    assert out[1][0].shape == (0, 2) and out[1][2].shape == (0,)
    assert not np.shares_memory(out[0][0], a)


def test_raise_with_counts():
    lib = types.SimpleNamespace(svo_last_error=lambda: b"image 1 has 9 key points, capacity 4")
    ctx = types.SimpleNamespace(lib=lib)
    n = (C.c_int * 4)(3, 9, 0, 77)
    with pytest.raises(capi.SvoError) as ei:
        capi._raise_with_counts(ctx, capi.SVO_ERR_CAPACITY, n, 3)
    err = ei.value
    assert err.code == capi.SVO_ERR_CAPACITY and err.needed == [3, 9, 0] and not hasattr(err, "prefix")
    assert str(err) == "libsvo_hip error -3: image 1 has 9 key points, capacity 4"
    with pytest.raises(capi.SvoError) as ei:
        capi._raise_with_counts(ctx, capi.SVO_ERR_CAPACITY, [3, 9, 0], 3, prefix=["rows"])
    assert ei.value.needed == [3, 9, 0] and ei.value.prefix == ["rows"]


def test_the_module_does_not_import_torch_at_import_time():
    text = pathlib.Path(capi.__file__).read_text()
    assert not re.search(r"^(import|from) torch", text, re.M)
    assert len(re.findall(r"^ +import torch$", text, re.M)) > 0
