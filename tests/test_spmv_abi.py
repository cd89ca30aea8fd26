"""Resident sparse matrices and the matrix-vector product at the boundary (no GPU): the four new symbols of include/msm_hip.h and
the two of its debug surface in the library and the binding, the enums, an unchanged ABI version and struct layout, and the
methods of the Python facade with its host helper."""
import ctypes as C

import pytest

from abi_surface import assert_abi_frozen, assert_header_declares, assert_prototypes, header_text, library

PROTOTYPES = {
    "msm_matrix_create": "msm_ctx* ctx, uint64_t rows, uint64_t cols, uint64_t nnz, const uint32_t* row_ptr, const uint32_t* col, "
                         "const void* val, int on_device, uint32_t flags, int32_t* id_out",
    "msm_matrix_destroy": "msm_ctx* ctx, int32_t id",
    "msm_matrix_info": "const msm_ctx* ctx, int32_t id, uint64_t* rows_out, uint64_t* cols_out, uint64_t* nnz_out, "
                       "uint64_t* bytes_out",
    "msm_scalars_matvec": "msm_ctx* ctx, int32_t id, void* dst, const void* x, const uint8_t* alpha, uint32_t flags",
    "msm_test_set_matvec_geometry": "msm_ctx* ctx, uint32_t short_max, uint32_t part_len",
    "msm_test_last_matvec": "msm_ctx* ctx, int32_t* out, int cap",
}


@pytest.fixture(scope="module")
def lib():
    return library()


def test_the_library_exports_the_symbols_with_the_declared_signatures(lib):
    from montgomery_amd import _lib

    assert_prototypes(lib, PROTOTYPES)
    # a null context is refused by every entry before anything else is looked at, and nothing is written
    out, word, big = (C.c_uint8 * 32)(*([7] * 32)), (C.c_int32 * 5)(7, 7, 7, 7, 7), [C.c_uint64(7) for _ in range(4)]
    rp, ident = (C.c_uint32 * 2)(0, 0), C.c_int32(7)
    assert lib.msm_matrix_create(None, 1, 1, 0, rp, None, None, 0, 0, C.byref(ident)) == _lib.MSM_ERR_ARG and ident.value == 7
    assert lib.msm_matrix_destroy(None, 1) == _lib.MSM_ERR_ARG
    assert lib.msm_matrix_info(None, 1, *[C.byref(b) for b in big]) == _lib.MSM_ERR_ARG
    assert [b.value for b in big] == [7, 7, 7, 7]
    assert lib.msm_scalars_matvec(None, 1, None, None, out, 0) == _lib.MSM_ERR_ARG and bytes(out) == bytes([7] * 32)
    assert lib.msm_test_set_matvec_geometry(None, 4, 64) == _lib.MSM_ERR_ARG
    assert lib.msm_test_last_matvec(None, word, 5) == -1 and list(word) == [7, 7, 7, 7, 7]


def test_abi_version_and_struct_sizes_are_unchanged(lib):
    assert_abi_frozen(lib)


def test_the_header_declares_the_symbols_and_the_enums():
    from montgomery_amd import _lib

    flat = assert_header_declares(PROTOTYPES)
    text = header_text()
    assert "enum { MSM_MATRIX_TRANSPOSE = 1 };" in flat and "enum { MSM_MATVEC_ACCUMULATE = 1 };" in flat
    assert (_lib.MATRIX_TRANSPOSE, _lib.MATVEC_ACCUMULATE) == (1, 1)
    # the contract a caller cannot guess: the aliasing rule, the determinism, and how a binding detects the feature
    assert "DISJOINT from x" in text and "THE RESULT IS THE SAME BITS WHATEVER THE LAUNCH GEOMETRY" in text
    assert "by the presence of msm_scalars_matvec" in text.replace("\n * ", " ")


def test_the_python_facade_has_the_methods_and_the_triplet_helper():
    from montgomery_amd import api

    for m in ("matrix_create", "matrix_destroy", "matrix_info", "scalars_matvec"):
        assert callable(getattr(api.MsmContext, m, None)), m
    for m in ("matrixCreate", "matrixDestroy", "matrixInfo", "scalarsMatvec", "matrixFromTriplets"):
        assert callable(getattr(api._Parallel, m, None)), m
    # the host helper: a stable sort over the rows, duplicates kept, values as 32 bytes; the transposed form; the all-ones form
    trip = [(2, 1, 5), (0, 3, 7), (2, 0, 6), (0, 3, 8), (2, 1, 9)]
    m = api.matrix_from_triplets(3, 4, trip)
    assert (m.rows, m.cols, m.nnz, m.row_ptr, m.col) == (3, 4, 5, [0, 2, 2, 5], [3, 3, 1, 0, 1])
    assert [int.from_bytes(m.val[32 * j:32 * j + 32], "little") for j in range(5)] == [7, 8, 5, 6, 9]
    t = api.matrix_from_triplets(3, 4, trip, transpose=True)
    assert (t.rows, t.cols, t.row_ptr, t.col) == (4, 3, [0, 1, 3, 3, 5], [2, 2, 2, 0, 0])
    assert [int.from_bytes(t.val[32 * j:32 * j + 32], "little") for j in range(5)] == [6, 5, 9, 7, 8]
    g = api.matrix_from_triplets(2, 2, [(1, 0), (0, 1), (1, 1)])
    assert (g.row_ptr, g.col, g.val) == ([0, 1, 3], [1, 0, 1], None)
    with pytest.raises(api.MsmError):
        api.matrix_from_triplets(2, 2, [(2, 0, 1)])
    with pytest.raises(api.MsmError):
        api.matrix_from_triplets(2, 2, [(0, 0, 1), (1, 1)])
