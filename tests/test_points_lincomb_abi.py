"""msm_points_lincomb / msm_pointset_size at the C ABI and in the Python binding, without a GPU: the two symbols, the unchanged
ABI version and struct sizes, and the argument handling of the facade that needs no device."""
import ctypes

import pytest

from abi_surface import abi_history, assert_abi_frozen, assert_names_declared

NAMES = ("msm_points_lincomb", "msm_pointset_size")


def test_header_binding_and_library_have_the_entries():
    assert_names_declared(NAMES)


def test_abi_version_and_struct_sizes_did_not_move():
    from montgomery_amd import _lib

    assert "msm_points_lincomb" in abi_history()                                  # the ABI-history comment says so
    assert_abi_frozen(_lib.load())


def test_null_context_is_an_argument_error():
    from montgomery_amd import _lib

    lib = _lib.load()
    one = (ctypes.c_uint8 * 32)(1)
    n = ctypes.c_uint64()
    assert lib.msm_points_lincomb(None, 0, 0, one, -1, 0, None, 1, 0) == _lib.MSM_ERR_ARG
    assert lib.msm_pointset_size(None, 0, ctypes.byref(n)) == _lib.MSM_ERR_ARG


def test_python_api_has_the_entries():
    from montgomery_amd import api

    for name in ("points_lincomb", "pointset_size", "fold_points"):
        assert callable(getattr(api.MsmContext, name))
    assert callable(api._Parallel.foldPoints) and callable(api._Parallel.pointsLincomb)


def test_scalars_are_checked_on_the_host():
    from montgomery_amd import api
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError

    assert api._scalar32(0) == bytes(32) and api._scalar32(1) == b"\x01" + bytes(31)
    assert api._scalar32((1 << 256) - 1) == b"\xff" * 32
    raw = bytes(range(32))
    assert api._scalar32(raw) == raw and api._scalar32(bytearray(raw)) == raw
    for bad in (1 << 256, -1, True, 1.5, "12", raw[:31], raw + b"\0", None):
        with pytest.raises(MsmError) as e:
            api._scalar32(bad)
        assert e.value.code == MSM_ERR_ARG


def test_facade_refuses_before_it_reaches_the_library():
    """The checks run before the context handle is touched: an object without one is enough to see them."""
    from montgomery_amd import api
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError

    ctx = api.MsmContext.__new__(api.MsmContext)   # no library call can succeed on this object
    ctx._h, ctx._lib, ctx.coord_bytes, ctx._cur_set, ctx.n_points, ctx._set_sizes = None, None, 48, 0, 5, {0: 5}
    calls = (
        lambda: ctx.points_lincomb(1 << 256),                       # scalar >= 2^256
        lambda: ctx.points_lincomb(3, 1 << 256),
        lambda: ctx.points_lincomb(-1),
        lambda: ctx.points_lincomb(bytes(31)),
        lambda: ctx.points_lincomb(3, 5, count=-1),                 # negative count
        lambda: ctx.points_lincomb(3, 5, a_lo=-1, count=1),
        lambda: ctx.points_lincomb(3, 5, b_lo=-2, count=1),
        lambda: ctx.fold_points(3, 5),                              # odd n
        lambda: ctx.fold_points(1 << 256, 5),
        lambda: ctx.fold_points(3, None),
    )
    for call in calls:
        with pytest.raises(MsmError) as e:
            call()
        assert e.value.code == MSM_ERR_ARG
    par = api._Parallel.__new__(api._Parallel)
    par._ctx = ctx
    ptr = api.PointPtr(None, n=4, set_id=0)
    with pytest.raises(MsmError) as e:
        par.pointsLincomb(ptr, 3, ptr, 5, None)                     # b without its pointer
    assert e.value.code == MSM_ERR_ARG
