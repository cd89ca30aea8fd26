"""The resident scans at the boundary (no GPU): the three new symbols of include/msm_hip.h and the two of its debug surface in the
library and the binding, the two enums, an unchanged ABI version and struct layout, and the methods of the Python facade."""
import ctypes as C

import pytest

from abi_surface import assert_abi_frozen, assert_header_declares, assert_prototypes, library

PROTOTYPES = {
    "msm_scalars_scan": "msm_ctx* ctx, void* dst, const void* a, uint64_t n, int op, uint32_t flags, const uint8_t* init, "
                        "uint8_t* total_out",
    "msm_scalars_inverse": "msm_ctx* ctx, void* dst, const void* a, uint64_t n, uint64_t* n_zero_out",
    "msm_scalars_div_linear": "msm_ctx* ctx, void* dst, const void* a, uint64_t n, const uint8_t* z, uint8_t* rem_out",
    "msm_test_set_scan_tile_log": "msm_ctx* ctx, int32_t tile_log",
    "msm_test_last_scan_plan": "msm_ctx* ctx, int32_t* tiles_out, int cap",
}


@pytest.fixture(scope="module")
def lib():
    return library()


def test_the_library_exports_the_symbols_with_the_declared_signatures(lib):
    from montgomery_amd import _lib

    assert_prototypes(lib, PROTOTYPES)
    # a null context is refused by every entry before anything else is looked at
    out, zeros = (C.c_uint8 * 32)(*([7] * 32)), C.c_uint64(7)
    assert lib.msm_scalars_scan(None, None, None, 0, _lib.SCAN_SUM, 0, None, out) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_inverse(None, None, None, 0, C.byref(zeros)) == _lib.MSM_ERR_ARG and zeros.value == 7
    assert lib.msm_scalars_div_linear(None, None, None, 0, out, out) == _lib.MSM_ERR_ARG
    assert bytes(out) == bytes([7] * 32)
    assert lib.msm_test_set_scan_tile_log(None, 8) == _lib.MSM_ERR_ARG
    assert lib.msm_test_last_scan_plan(None, None, 0) == -1


def test_abi_version_and_struct_sizes_are_unchanged(lib):
    assert_abi_frozen(lib)


def test_the_header_declares_the_symbols_and_the_enums():
    from montgomery_amd import _lib

    flat = assert_header_declares(PROTOTYPES)
    assert "enum { MSM_SCAN_SUM = 0, MSM_SCAN_PRODUCT = 1 };" in flat and (_lib.SCAN_SUM, _lib.SCAN_PRODUCT) == (0, 1)
    assert "enum { MSM_SCAN_EXCLUSIVE = 1 };" in flat and _lib.SCAN_EXCLUSIVE == 1


def test_the_python_facade_has_the_methods():
    from montgomery_amd import api

    for m in ("scalars_scan", "scalars_inverse", "scalars_div_linear"):
        assert callable(getattr(api.MsmContext, m, None)), m
    for m in ("scalarsScan", "scalarsInverse", "scalarsDivLinear"):
        assert callable(getattr(api._Parallel, m, None)), m
