"""msm_run_batch at the C ABI and in the bindings, without a GPU: the symbol, its argument checks, the addon's exports."""
import ctypes

from napi_support import assert_exports


def test_library_exports_msm_run_batch():
    from montgomery_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "msm_run_batch")
    assert "msm_run_batch" in _lib.EXPORTS
    assert _lib.ABI_VERSION >= 7


def test_msm_run_batch_without_context_is_an_argument_error():
    from montgomery_amd import _lib
    from montgomery_amd._lib import MsmOpts, MsmResult

    lib = _lib.load()
    s = (ctypes.c_uint8 * 64)()
    arr = (ctypes.c_void_p * 1)(ctypes.cast(s, ctypes.c_void_p))
    res = (MsmResult * 1)()
    o = MsmOpts()
    assert lib.msm_run_batch(None, arr, 1, 2, 0, ctypes.byref(o), res) == _lib.MSM_ERR_ARG
    assert lib.msm_run_batch(None, None, 0, 0, 0, None, None) == _lib.MSM_ERR_ARG


def test_python_api_has_the_batch_entries():
    from montgomery_amd import api

    assert callable(api.MsmContext.run_batch) and callable(api.MsmContext.run_batch_device)
    assert callable(api._Parallel.msmBatch)


def test_addon_exports_batch_entries():
    assert_exports(("msmBatch", "msmBatchDevice"), facade=())
