"""The resident scans at the boundary (no GPU): the three new symbols of include/msm_hip.h and the two of its debug surface in the
library and the binding, the two enums, an unchanged ABI version and struct layout, and the methods of the Python facade."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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
    from conftest import build_if_missing

    build_if_missing("all", "montgomery_amd/libmsm_hip.so")
    from montgomery_amd import _lib

    return _lib.load()


def test_the_library_exports_the_symbols_with_the_declared_signatures(lib):
    from montgomery_amd import _lib

    for name, args in PROTOTYPES.items():
        assert name in _lib.EXPORTS, name
        fn = getattr(lib, name)                      # AttributeError: the library has no such symbol
        assert len(fn.argtypes) == args.count(",") + 1 and fn.restype is C.c_int, name
    # a null context is refused by every entry before anything else is looked at
    out, zeros = (C.c_uint8 * 32)(*([7] * 32)), C.c_uint64(7)
    assert lib.msm_scalars_scan(None, None, None, 0, _lib.SCAN_SUM, 0, None, out) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_inverse(None, None, None, 0, C.byref(zeros)) == _lib.MSM_ERR_ARG and zeros.value == 7
    assert lib.msm_scalars_div_linear(None, None, None, 0, out, out) == _lib.MSM_ERR_ARG
    assert bytes(out) == bytes([7] * 32)
    assert lib.msm_test_set_scan_tile_log(None, 8) == _lib.MSM_ERR_ARG
    assert lib.msm_test_last_scan_plan(None, None, 0) == -1


def test_abi_version_and_struct_sizes_are_unchanged(lib):
    from montgomery_amd import _lib

    assert lib.msm_abi_version() == 8 == _lib.ABI_VERSION
    assert lib.msm_abi_struct_bytes(0) == 56 == C.sizeof(_lib.MsmOpts)
    assert lib.msm_abi_struct_bytes(1) == 176 == C.sizeof(_lib.MsmResult)


def test_the_header_declares_the_symbols_and_the_enums():
    from montgomery_amd import _lib

    text = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    assert re.search(r"#define\s+MSM_ABI_VERSION\s+8\b", text)
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)          # comments out, then one space between tokens
    flat = re.sub(r"\s+", " ", flat).replace("( ", "(").replace(" )", ")").replace(" ,", ",")
    for name, args in PROTOTYPES.items():
        assert f"int {name}({args});" in flat, name
    assert "enum { MSM_SCAN_SUM = 0, MSM_SCAN_PRODUCT = 1 };" in flat and (_lib.SCAN_SUM, _lib.SCAN_PRODUCT) == (0, 1)
    assert "enum { MSM_SCAN_EXCLUSIVE = 1 };" in flat and _lib.SCAN_EXCLUSIVE == 1


def test_the_python_facade_has_the_methods():
    from montgomery_amd import api

    for m in ("scalars_scan", "scalars_inverse", "scalars_div_linear"):
        assert callable(getattr(api.MsmContext, m, None)), m
    for m in ("scalarsScan", "scalarsInverse", "scalarsDivLinear"):
        assert callable(getattr(api._Parallel, m, None)), m
