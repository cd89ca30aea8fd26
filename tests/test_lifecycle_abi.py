"""The count of live device buffers at the boundary (no GPU): the one new symbol of the debug surface in the header, the library
and the binding, an unchanged ABI version and struct layout, the refusal of null outputs, and the reading of a process that never
created a context."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "msm_test_live_buffers": "uint64_t* count_out, uint64_t* bytes_out",
}


@pytest.fixture(scope="module")
def lib():
    from conftest import build_if_missing

    build_if_missing("all", "montgomery_amd/libmsm_hip.so")
    from montgomery_amd import _lib

    return _lib.load()


def test_the_library_exports_the_symbol_with_the_declared_signature(lib):
    from montgomery_amd import _lib, api

    for name, args in PROTOTYPES.items():
        assert name in _lib.EXPORTS, name
        fn = getattr(lib, name)                      # AttributeError: the library has no such symbol
        assert len(fn.argtypes) == args.count(",") + 1 and fn.restype is C.c_int, name
    assert callable(getattr(api.MsmContext, "test_live_buffers", None))
    # null outputs are refused, whichever of the two it is, and nothing is written
    count, nbytes = C.c_uint64(7), C.c_uint64(7)
    assert lib.msm_test_live_buffers(None, None) == _lib.MSM_ERR_ARG
    assert lib.msm_test_live_buffers(C.byref(count), None) == _lib.MSM_ERR_ARG
    assert lib.msm_test_live_buffers(None, C.byref(nbytes)) == _lib.MSM_ERR_ARG
    assert (count.value, nbytes.value) == (7, 7)


def test_abi_version_and_struct_sizes_are_unchanged(lib):
    from montgomery_amd import _lib

    assert lib.msm_abi_version() == 8 == _lib.ABI_VERSION
    assert lib.msm_abi_struct_bytes(0) == 56 == C.sizeof(_lib.MsmOpts)
    assert lib.msm_abi_struct_bytes(1) == 176 == C.sizeof(_lib.MsmResult)


def test_the_header_declares_the_symbol():
    text = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    assert re.search(r"#define\s+MSM_ABI_VERSION\s+8\b", text)
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)          # comments out, then one space between tokens
    flat = re.sub(r"\s+", " ", flat).replace("( ", "(").replace(" )", ")").replace(" ,", ",")
    for name, args in PROTOTYPES.items():
        assert f"int {name}({args});" in flat, name


def test_a_process_that_never_created_a_context_reads_zero(lib):
    """A process of its own: this one may hold the contexts of other tests."""
    code = "from montgomery_amd.api import MsmContext; print(MsmContext.test_live_buffers())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "(0, 0)"
