"""msm_points_ntt at the C ABI and in the Python binding, without a GPU: the symbols, the unchanged ABI version and struct sizes,
the History comment, and the argument handling that needs no device.  The refusals that need a live context (bad ids, log2n too
large, omega of the wrong order, a shift of 0, a range beyond the set, a forbidden overlap, a device-list context, a failed call
leaving every set as it was) are in tests/test_gpu_points_ntt.py::test_every_refusal_leaves_the_sets_as_they_were."""
import ctypes

import pytest

from abi_surface import abi_history, assert_abi_frozen, assert_names_declared

NAMES = ("msm_points_ntt", "msm_test_set_points_ntt_grid", "msm_test_last_points_ntt")


def test_header_binding_and_library_have_the_entries():
    from montgomery_amd import _lib

    assert_names_declared(NAMES)
    bound = _lib.load()
    assert bound.msm_points_ntt.argtypes is not None and len(bound.msm_points_ntt.argtypes) == 8


def test_abi_version_and_struct_sizes_did_not_move():
    from montgomery_amd import _lib

    assert "msm_points_ntt" in abi_history()                                      # the ABI-history comment says so
    assert_abi_frozen(_lib.load())


def test_null_context_is_an_argument_error():
    from montgomery_amd import _lib

    lib = _lib.load()
    out = (ctypes.c_int32 * 7)()
    assert lib.msm_points_ntt(None, 0, 0, 3, None, None, 0, 0) == _lib.MSM_ERR_ARG
    assert lib.msm_test_set_points_ntt_grid(None, 1) == _lib.MSM_ERR_ARG
    assert lib.msm_test_last_points_ntt(None, out, 7) == -1


def test_python_api_has_the_entry():
    import inspect

    from montgomery_amd import api

    sig = inspect.signature(api.MsmContext.points_ntt)
    assert list(sig.parameters)[1:] == ["src", "a_lo", "log2n", "omega", "shift", "inverse", "dst"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[1:])


def test_facade_refuses_before_it_reaches_the_library():
    """The checks run before the context handle is touched: an object without one is enough to see them."""
    from montgomery_amd import api
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError

    ctx = api.MsmContext.__new__(api.MsmContext)   # no library call can succeed on this object
    ctx._h, ctx._lib, ctx.coord_bytes, ctx._cur_set, ctx.n_points, ctx._set_sizes = None, None, 48, 0, 8, {0: 8}
    for call in (lambda: ctx.points_ntt(log2n=-1), lambda: ctx.points_ntt(log2n=2, a_lo=-1)):
        with pytest.raises(MsmError) as e:
            call()
        assert e.value.code == MSM_ERR_ARG
