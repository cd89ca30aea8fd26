"""The count of live device buffers at the boundary (no GPU): the one new symbol of the debug surface in the header, the library
and the binding, an unchanged ABI version and struct layout, the refusal of null outputs, and the reading of a process that never
created a context."""
import ctypes as C
import subprocess
import sys

import pytest

from abi_surface import ROOT, assert_abi_frozen, assert_header_declares, assert_prototypes, library

PROTOTYPES = {
    "msm_test_live_buffers": "uint64_t* count_out, uint64_t* bytes_out",
}


@pytest.fixture(scope="module")
def lib():
    return library()


def test_the_library_exports_the_symbol_with_the_declared_signature(lib):
    from montgomery_amd import _lib, api

    assert_prototypes(lib, PROTOTYPES)
    assert callable(getattr(api.MsmContext, "test_live_buffers", None))
    # null outputs are refused, whichever of the two it is, and nothing is written
    count, nbytes = C.c_uint64(7), C.c_uint64(7)
    assert lib.msm_test_live_buffers(None, None) == _lib.MSM_ERR_ARG
    assert lib.msm_test_live_buffers(C.byref(count), None) == _lib.MSM_ERR_ARG
    assert lib.msm_test_live_buffers(None, C.byref(nbytes)) == _lib.MSM_ERR_ARG
    assert (count.value, nbytes.value) == (7, 7)


def test_abi_version_and_struct_sizes_are_unchanged(lib):
    assert_abi_frozen(lib)


def test_the_header_declares_the_symbol():
    assert_header_declares(PROTOTYPES)


def test_a_process_that_never_created_a_context_reads_zero(lib):
    """A process of its own: this one may hold the contexts of other tests."""
    code = "from montgomery_amd.api import MsmContext; print(MsmContext.test_live_buffers())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "(0, 0)"
