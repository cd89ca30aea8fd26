"""The resident scalar-vector operations at the boundary (no GPU): the five new symbols of include/msm_hip.h in the library and
the binding, an unchanged ABI version and struct layout, and the methods of the Python facade."""
import pytest

from abi_surface import assert_abi_frozen, assert_header_declares, assert_prototypes, library

PROTOTYPES = {
    "msm_device_download": "msm_ctx* ctx, void* host, const void* dev_ptr, uint64_t bytes",
    "msm_scalars_lincomb": "msm_ctx* ctx, void* dst, const uint8_t* x, const void* a, const uint8_t* y, const void* b, uint64_t n",
    "msm_scalars_mul": "msm_ctx* ctx, void* dst, const void* a, const void* b, uint64_t n",
    "msm_scalars_inner": "msm_ctx* ctx, const void* a, const void* b, uint64_t n, uint8_t* out",
    "msm_scalars_powers": "msm_ctx* ctx, void* dst, const uint8_t* s, const uint8_t* x, uint64_t n",
}


@pytest.fixture(scope="module")
def lib():
    return library()


def test_the_library_exports_the_symbols_with_the_declared_signatures(lib):
    from montgomery_amd import _lib

    assert_prototypes(lib, PROTOTYPES)
    # a null context is refused by every entry before anything else is looked at
    assert lib.msm_device_download(None, None, None, 0) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_lincomb(None, None, None, None, None, None, 0) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_mul(None, None, None, None, 0) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_inner(None, None, None, 0, None) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_powers(None, None, None, None, 0) == _lib.MSM_ERR_ARG


def test_abi_version_and_struct_sizes_are_unchanged(lib):
    assert_abi_frozen(lib)


def test_the_header_declares_the_symbols():
    assert_header_declares(PROTOTYPES)


def test_the_python_facade_has_the_methods():
    from montgomery_amd import api

    for m in ("device_download", "scalars_lincomb", "scalars_mul", "scalars_inner", "scalars_powers", "fold_scalars"):
        assert callable(getattr(api.MsmContext, m, None)), m
    for m in ("scalarsLincomb", "scalarsMul", "scalarsInner", "scalarsPowers", "foldScalars"):
        assert callable(getattr(api._Parallel, m, None)), m
