"""The resident sumcheck at the boundary (no GPU): the three new symbols of include/msm_hip.h and the two of its debug surface in
the library and the binding, the enum, an unchanged ABI version and struct layout, and the methods of the Python facade."""
import ctypes as C

import pytest

from abi_surface import assert_abi_frozen, assert_header_declares, assert_prototypes, header_text, library

PROTOTYPES = {
    "msm_scalars_sumcheck_round": "msm_ctx* ctx, const void* const* vecs, uint32_t m, uint32_t log2n, uint32_t var, int shape, "
                                  "uint8_t* evals_out",
    "msm_scalars_bind": "msm_ctx* ctx, void* const* dst, const void* const* a, uint32_t m, uint32_t log2n, uint32_t var, "
                        "const uint8_t* r",
    "msm_scalars_eq": "msm_ctx* ctx, void* dst, const uint8_t* r, uint32_t v, const uint8_t* s",
    "msm_test_set_sumcheck_grid": "msm_ctx* ctx, int32_t blocks",
    "msm_test_last_sumcheck": "msm_ctx* ctx, int32_t* out, int cap",
}


@pytest.fixture(scope="module")
def lib():
    return library()


def test_the_library_exports_the_symbols_with_the_declared_signatures(lib):
    from montgomery_amd import _lib

    assert_prototypes(lib, PROTOTYPES)
    # a null context is refused by every entry before anything else is looked at, and nothing is written
    out, word = (C.c_uint8 * 160)(*([7] * 160)), (C.c_int32 * 4)(7, 7, 7, 7)
    vecs = (C.c_void_p * 4)()
    assert lib.msm_scalars_sumcheck_round(None, vecs, 2, 4, 0, _lib.SUMCHECK_PROD, out) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_bind(None, vecs, vecs, 1, 4, 3, out) == _lib.MSM_ERR_ARG
    assert lib.msm_scalars_eq(None, None, out, 2, out) == _lib.MSM_ERR_ARG
    assert bytes(out) == bytes([7] * 160)
    assert lib.msm_test_set_sumcheck_grid(None, 3) == _lib.MSM_ERR_ARG
    assert lib.msm_test_last_sumcheck(None, word, 4) == -1 and list(word) == [7, 7, 7, 7]


def test_abi_version_and_struct_sizes_are_unchanged(lib):
    assert_abi_frozen(lib)


def test_the_header_declares_the_symbols_and_the_enum():
    from montgomery_amd import _lib

    flat = assert_header_declares(PROTOTYPES)
    text = header_text()
    assert "enum { MSM_SUMCHECK_PROD = 0, MSM_SUMCHECK_R1CS = 1 };" in flat
    assert (_lib.SUMCHECK_PROD, _lib.SUMCHECK_R1CS) == (0, 1)
    # the contract a caller cannot guess: which bit a variable is, and what to do with a sum of products
    assert "VARIABLE j IS BIT j OF THE INDEX" in text and "least significant bit" in text
    assert "linear in g" in text and "one call per product" in text


def test_the_python_facade_has_the_methods():
    from montgomery_amd import api

    for m in ("scalars_sumcheck_round", "scalars_bind", "scalars_eq"):
        assert callable(getattr(api.MsmContext, m, None)), m
    for m in ("scalarsSumcheckRound", "scalarsBind", "scalarsEq"):
        assert callable(getattr(api._Parallel, m, None)), m
