"""The resident NTT at the boundary (no GPU): the three new symbols of include/msm_hip.h and the two of its debug surface in the
library and the binding, an unchanged ABI version and struct layout, the methods of the Python facade, and the host-only entries
(the root of unity and the size limit need no device work, so a context handle is all they would need -- here: their refusals)."""
import ctypes as C

import pytest

from abi_surface import assert_abi_frozen, assert_header_declares, assert_prototypes, library

PROTOTYPES = {
    "msm_scalars_ntt": "msm_ctx* ctx, void* dst, const void* a, uint32_t log2n, uint32_t B, const uint8_t* omega, const uint8_t* shift, "
                       "int inverse",
    "msm_scalars_root_of_unity": "const msm_ctx* ctx, uint32_t log2n, uint8_t* out",
    "msm_scalars_ntt_max_log2n": "const msm_ctx* ctx, uint32_t* out",
    "msm_test_set_ntt_tile_log": "msm_ctx* ctx, int32_t tile_log",
    "msm_test_last_ntt_plan": "msm_ctx* ctx, int32_t* stages_out, int cap",
}


@pytest.fixture(scope="module")
def lib():
    return library()


def test_the_library_exports_the_symbols_with_the_declared_signatures(lib):
    from montgomery_amd import _lib

    assert_prototypes(lib, PROTOTYPES)
    # a null context is refused by every entry before anything else is looked at
    out, top = (C.c_uint8 * 32)(), C.c_uint32(7)
    assert lib.msm_scalars_ntt(None, None, None, 0, 1, None, None, 0) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_root_of_unity(None, 0, out) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_ntt_max_log2n(None, C.byref(top)) == _lib.MSM_ERR_ARG and top.value == 7
    assert lib.msm_test_set_ntt_tile_log(None, 3) == _lib.MSM_ERR_ARG
    assert lib.msm_test_last_ntt_plan(None, None, 0) == -1


def test_abi_version_and_struct_sizes_are_unchanged(lib):
    assert_abi_frozen(lib)


def test_the_header_declares_the_symbols():
    assert_header_declares(PROTOTYPES)


def test_the_python_facade_has_the_methods():
    from montgomery_amd import api

    for m in ("scalars_ntt", "scalars_root_of_unity", "scalars_ntt_max_log2n"):
        assert callable(getattr(api.MsmContext, m, None)), m
    for m in ("scalarsNtt", "scalarsRootOfUnity"):
        assert callable(getattr(api._Parallel, m, None)), m
