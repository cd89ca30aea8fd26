"""The resident scalar-vector operations at the boundary (no GPU): the five new symbols of include/msm_hip.h in the library and
the binding, an unchanged ABI version and struct layout, and the methods of the Python facade."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> number of arguments of its prototype
SYMBOLS = {
    "msm_device_download": 4,
    "msm_scalars_lincomb": 7,
    "msm_scalars_mul": 5,
    "msm_scalars_inner": 5,
    "msm_scalars_powers": 5,
}
PROTOTYPES = {
    "msm_device_download": "msm_ctx* ctx, void* host, const void* dev_ptr, uint64_t bytes",
    "msm_scalars_lincomb": "msm_ctx* ctx, void* dst, const uint8_t* x, const void* a, const uint8_t* y, const void* b, uint64_t n",
    "msm_scalars_mul": "msm_ctx* ctx, void* dst, const void* a, const void* b, uint64_t n",
    "msm_scalars_inner": "msm_ctx* ctx, const void* a, const void* b, uint64_t n, uint8_t* out",
    "msm_scalars_powers": "msm_ctx* ctx, void* dst, const uint8_t* s, const uint8_t* x, uint64_t n",
}


@pytest.fixture(scope="module")
def lib():
    from conftest import build_if_missing

    build_if_missing("all", "montgomery_amd/libmsm_hip.so")
    from montgomery_amd import _lib

    return _lib.load()


def test_the_library_exports_the_symbols_with_the_declared_signatures(lib):
    from montgomery_amd import _lib

    for name, n_args in SYMBOLS.items():
        assert name in _lib.EXPORTS, name
        fn = getattr(lib, name)                      # AttributeError: the library has no such symbol
        assert len(fn.argtypes) == n_args and fn.restype is C.c_int, name
    # a null context is refused by every entry before anything else is looked at
    assert lib.msm_device_download(None, None, None, 0) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_lincomb(None, None, None, None, None, None, 0) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_mul(None, None, None, None, 0) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_inner(None, None, None, 0, None) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_powers(None, None, None, None, 0) == _lib.MSM_ERR_ARG


def test_abi_version_and_struct_sizes_are_unchanged(lib):
    from montgomery_amd import _lib

    assert lib.msm_abi_version() == 8 == _lib.ABI_VERSION
    assert lib.msm_abi_struct_bytes(0) == 56 == C.sizeof(_lib.MsmOpts)
    assert lib.msm_abi_struct_bytes(1) == 176 == C.sizeof(_lib.MsmResult)


def test_the_header_declares_the_symbols():
    text = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    assert re.search(r"#define\s+MSM_ABI_VERSION\s+8\b", text)
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)          # comments out, then one space between tokens
    flat = re.sub(r"\s+", " ", flat).replace("( ", "(").replace(" )", ")").replace(" ,", ",")
    for name, args in PROTOTYPES.items():
        assert f"int {name}({args});" in flat, name


def test_the_python_facade_has_the_methods():
    from montgomery_amd import api

    for m in ("device_download", "scalars_lincomb", "scalars_mul", "scalars_inner", "scalars_powers", "fold_scalars"):
        assert callable(getattr(api.MsmContext, m, None)), m
    for m in ("scalarsLincomb", "scalarsMul", "scalarsInner", "scalarsPowers", "foldScalars"):
        assert callable(getattr(api._Parallel, m, None)), m
