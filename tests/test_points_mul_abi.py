"""msm_points_mul / msm_points_mul_base at the C ABI and in the Python binding, without a GPU: the symbols, the unchanged ABI
version and struct sizes, the History comment, and the argument handling that needs no device.  The error classes that need a
live context (bad ids, misaligned device scalars, the forbidden overlap, a source range beyond the set, an off-curve base, a
failed call leaving every set as it was) are in tests/test_gpu_points_mul.py::test_every_refusal_leaves_the_sets_as_they_were."""
import ctypes

import pytest

from abi_surface import abi_history, assert_abi_frozen, assert_names_declared

NAMES = ("msm_points_mul", "msm_points_mul_base", "msm_test_set_points_mul_grid", "msm_test_set_points_mul_base_path",
         "msm_test_last_points_mul")


def test_header_binding_and_library_have_the_entries():
    from montgomery_amd import _lib

    assert_names_declared(NAMES)
    bound = _lib.load()
    assert bound.msm_points_mul.argtypes is not None and len(bound.msm_points_mul.argtypes) == 7
    assert bound.msm_points_mul_base.argtypes is not None and len(bound.msm_points_mul_base.argtypes) == 6


def test_abi_version_and_struct_sizes_did_not_move():
    from montgomery_amd import _lib

    history = abi_history()
    assert "msm_points_mul" in history and "msm_points_mul_base" in history     # the ABI-history comment says so
    assert_abi_frozen(_lib.load())


def test_null_context_is_an_argument_error():
    from montgomery_amd import _lib

    lib = _lib.load()
    s = (ctypes.c_uint8 * 32)(1)
    out = (ctypes.c_int32 * 4)()
    assert lib.msm_points_mul(None, 0, 0, s, 0, 1, 0) == _lib.MSM_ERR_ARG
    assert lib.msm_points_mul_base(None, None, s, 0, 1, 0) == _lib.MSM_ERR_ARG
    assert lib.msm_test_set_points_mul_grid(None, 1) == _lib.MSM_ERR_ARG
    assert lib.msm_test_set_points_mul_base_path(None, 1) == _lib.MSM_ERR_ARG
    assert lib.msm_test_last_points_mul(None, out, 4) == -1


def test_python_api_has_the_entries():
    from montgomery_amd import api

    for name in ("points_mul", "points_mul_base"):
        assert callable(getattr(api.MsmContext, name))


def test_facade_refuses_before_it_reaches_the_library():
    """The checks run before the context handle is touched: an object without one is enough to see them."""
    from montgomery_amd import api
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError

    ctx = api.MsmContext.__new__(api.MsmContext)   # no library call can succeed on this object
    ctx._h, ctx._lib, ctx.coord_bytes, ctx._cur_set, ctx.n_points, ctx._set_sizes = None, None, 48, 0, 5, {0: 5}
    two = bytes(64)
    calls = (
        lambda: ctx.points_mul(bytes(31)),                          # not a multiple of 32 bytes
        lambda: ctx.points_mul(two, count=3),                       # more rows than scalars
        lambda: ctx.points_mul(two, count=-1),
        lambda: ctx.points_mul(two, a_lo=-1),
        lambda: ctx.points_mul(0x1000),                             # a device address without count
        lambda: ctx.points_mul(None),
        lambda: ctx.points_mul(True),
        lambda: ctx.points_mul_base(bytes(33)),
        lambda: ctx.points_mul_base(two, count=3),
        lambda: ctx.points_mul_base(0x1000),
        lambda: ctx.points_mul_base(two, bytes(95)),                # a base that is not x || y
        lambda: ctx.points_mul_base(two, bytes(64)),
    )
    for call in calls:
        with pytest.raises(MsmError) as e:
            call()
        assert e.value.code == MSM_ERR_ARG


def test_scalar_vectors_of_every_accepted_kind():
    import numpy as np

    from montgomery_amd import api

    raw = bytes(range(64))
    for v in (raw, bytearray(raw), memoryview(raw), (ctypes.c_uint8 * 64).from_buffer_copy(raw),
              np.frombuffer(raw, dtype=np.uint8), np.frombuffer(raw, dtype=np.uint32).reshape(2, 8)):
        buf, on_device, count, _ = api.MsmContext._scalar_vector(v, None, "t")
        assert (on_device, count) == (0, 2) and bytes(buf)[:64] == raw
    ptr, on_device, count, _ = api.MsmContext._scalar_vector(0x7F0000001000, 5, "t")
    assert (ptr.value, on_device, count) == (0x7F0000001000, 1, 5)
    assert api.MsmContext._scalar_vector(raw, 1, "t")[2] == 1
    assert api.MsmContext._scalar_vector(b"", None, "t")[2] == 0
