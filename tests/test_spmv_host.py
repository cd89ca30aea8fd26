"""The CSR rule, the plan of the long rows, the host transposition and the lane bodies of montgomery_amd/csrc/scalar_spmv.h on the
CPU (tests/csrc/spmv_host.hip), the lane bodies over the scalar field the dispatch gives each of the seven curves, bit for bit
against Python integers mod cv.q.

Elements are raw 256-bit integers -- an element >= q stands for its residue -- and every result must be canonical.  The edge
operands (0, 1, q - 1, q, q + 1, 2^256 - 1) in every pairing of coefficient, x and old dst, with alpha absent, 0, 1 and q - 1,
drive the value bounds written in the header of scalar_spmv.h to their ends, on the 251-bit modulus of Ed-on-BLS12-377 as on the
255-bit ones.  The plan is compared with part lists derived by hand at the thresholds (4, 64)."""
import ctypes as C
import itertools
import os
import random
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402

from host_lib import host_library, value, vec, words  # noqa: E402
from operator_fixture import TOP, edges  # noqa: E402

FIN_ALPHA, FIN_ACCUMULATE = 1, 2


@pytest.fixture(scope="module")
def lib():
    L = host_library("spmv_host")
    u32p = C.POINTER(C.c_uint32)
    L.spmv_row.argtypes = [C.c_int, C.c_int, C.c_int, u32p, u32p, C.c_int, C.c_uint32, u32p, u32p, u32p]
    L.spmv_value.argtypes = [C.c_int, u32p, u32p]
    L.spmv_plan.argtypes = [u32p, C.c_uint64, C.c_uint32, C.c_uint32, u32p, C.c_int, u32p, u32p, C.POINTER(C.c_int)]
    L.spmv_check.argtypes = [u32p, u32p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), u32p, C.c_char_p, C.c_int]
    L.spmv_row_ptr_entry_ok.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
    L.spmv_col_entry_ok.argtypes = [C.c_uint32, C.c_uint64]
    L.spmv_transpose.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u32p, u32p, u32p, u32p, u32p, u32p]
    L.spmv_transpose.restype = None
    return L


def u32(vals):
    return (C.c_uint32 * max(len(vals), 1))(*vals)


def row(lib, cv, coef, x, cut=None, alpha=None, old=None, ones=False):
    """one row through the shim: -> the canonical word it stores"""
    n = len(x)
    mode = (FIN_ALPHA if alpha is not None else 0) | (FIN_ACCUMULATE if old is not None else 0)
    out = (C.c_uint32 * 8)()
    assert lib.spmv_row(cv.cid, int(ones), n, vec(coef if not ones else []), vec(x), n if cut is None else cut, mode,
                        words(alpha or 0), words(old or 0), out) == 0
    return value(out)


def expect(q, coef, x, alpha=None, old=None):
    s = sum(c * v for c, v in zip(coef, x))
    return ((1 if alpha is None else alpha) * s + (old or 0)) % q


# ---------------------------------------------------------------------------------------------- the lane bodies

@pytest.mark.parametrize("name", D.NAMES)
def test_the_term_the_combine_and_the_three_finishes_on_edge_operands(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    E = edges(q)
    for alpha in (None, 0, 1, q - 1):
        for c, x in itertools.product(E, E):
            # a lone term, finished without and with every old dst
            assert row(lib, cv, [c], [x], alpha=alpha) == expect(q, [c], [x], alpha), (name, alpha, c, x)
            for old in E:
                assert row(lib, cv, [c], [x], alpha=alpha, old=old) == expect(q, [c], [x], alpha, old), (name, alpha, c, x, old)
            # the all-ones form: no coefficient is read
            assert row(lib, cv, None, [x], alpha=alpha, old=c, ones=True) == expect(q, [1], [x], alpha, c)
        # all 36 pairings in one row, cut into a lane's share and a partial at every sixth place
        coef = [c for c in E for _ in E]
        xs = [x for _ in E for x in E]
        for cut in (0, 6, 17, 36):
            assert row(lib, cv, coef, xs, cut=cut, alpha=alpha, old=TOP) == expect(q, coef, xs, alpha, TOP), (name, alpha, cut)
            assert row(lib, cv, None, xs, cut=cut, alpha=alpha, ones=True) == expect(q, [1] * 36, xs, alpha)
    # the empty row
    for alpha in (None, 0, q - 1):
        assert row(lib, cv, [], [], alpha=alpha) == 0
        for old in E:
            assert row(lib, cv, [], [], alpha=alpha, old=old) == old % q


@pytest.mark.parametrize("name", D.NAMES)
def test_a_coefficient_goes_to_canonical_montgomery_form(lib, name):
    cv = D.CURVE_TABLE[name]
    q, R = cv.q, 1 << 270
    rng = random.Random(f"spmv/value/{name}")
    for v in edges(q) + [rng.randrange(1 << 256) for _ in range(20)]:
        out = (C.c_uint32 * 8)()
        assert lib.spmv_value(cv.cid, words(v), out) == 0
        assert value(out) == v * R % q, (name, v)


@pytest.mark.parametrize("name", D.NAMES)
def test_random_rows_do_not_depend_on_the_cut(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    rng = random.Random(f"spmv/rows/{name}")
    for n in (1, 2, 5, 64, 130):
        coef = [rng.randrange(1 << 256) for _ in range(n)]
        xs = [rng.randrange(1 << 256) for _ in range(n)]
        alpha, old = rng.randrange(q), rng.randrange(1 << 256)
        want = expect(q, coef, xs, alpha, old)
        for cut in sorted({0, 1, n // 2, n}):
            assert row(lib, cv, coef, xs, cut=cut, alpha=alpha, old=old) == want, (name, n, cut)


# ---------------------------------------------------------------------------------------------- the plan

def plan(lib, lens, short_max, part_len):
    """row lengths -> (parts as (row, first, len), long rows, long_first)"""
    rp = [0]
    for n in lens:
        rp.append(rp[-1] + n)
    cap = sum(-(-n // part_len) for n in lens) + 1
    parts, lr, lf, nl = (C.c_uint32 * (3 * cap))(), (C.c_uint32 * (len(lens) + 1))(), (C.c_uint32 * (len(lens) + 2))(), C.c_int(-1)
    n = lib.spmv_plan(u32(rp), len(lens), short_max, part_len, parts, cap, lr, lf, C.byref(nl))
    assert 0 <= n < cap
    return ([(parts[3 * p], parts[3 * p + 1], parts[3 * p + 2]) for p in range(n)], list(lr[:nl.value]), list(lf[:nl.value + 1]))


def test_the_plan_against_hand_derived_part_lists(lib):
    # thresholds (4, 64): rows of 0, 4 and 5 entries; 5 > 4 is long and one part
    assert plan(lib, [0, 4, 5], 4, 64) == ([(2, 4, 5)], [2], [0, 1])
    # 63, 64, 65, 128, 129 entries: firsts 0, 63, 127, 192, 320
    assert plan(lib, [63, 64, 65, 128, 129], 4, 64) == (
        [(0, 0, 63), (1, 63, 64), (2, 127, 64), (2, 191, 1), (3, 192, 64), (3, 256, 64), (4, 320, 64), (4, 384, 64), (4, 448, 1)],
        [0, 1, 2, 3, 4], [0, 1, 2, 4, 6, 9])
    # 5 * 64 + 3 entries behind a short row of 2
    assert plan(lib, [2, 323], 4, 64) == (
        [(1, 2, 64), (1, 66, 64), (1, 130, 64), (1, 194, 64), (1, 258, 64), (1, 322, 3)], [1], [0, 6])
    # a long row first, last, and alone
    assert plan(lib, [70, 1, 2], 4, 64) == ([(0, 0, 64), (0, 64, 6)], [0], [0, 2])
    assert plan(lib, [1, 2, 70], 4, 64) == ([(2, 3, 64), (2, 67, 6)], [2], [0, 2])
    assert plan(lib, [70], 4, 64) == ([(0, 0, 64), (0, 64, 6)], [0], [0, 2])
    # no long row at all, and no row at all
    assert plan(lib, [0, 1, 2, 3, 4, 4, 0], 4, 64) == ([], [], [0])
    assert plan(lib, [], 4, 64) == ([], [], [0])
    # part_len below short_max, and both 1: every entry of a row of two or more is a part
    assert plan(lib, [5], 4, 2) == ([(0, 0, 2), (0, 2, 2), (0, 4, 1)], [0], [0, 3])
    assert plan(lib, [1, 2, 0, 3], 1, 1) == ([(1, 1, 1), (1, 2, 1), (3, 3, 1), (3, 4, 1), (3, 5, 1)], [1, 3], [0, 2, 5])


def test_the_parts_tile_every_long_row_exactly_once_in_order(lib):
    rng = random.Random("spmv/plan")
    for short_max, part_len in itertools.product((1, 4, 7, 32), (1, 5, 64, 96)):
        for trial in range(6):
            lens = [rng.choice((0, 1, short_max, short_max + 1, part_len, part_len + 1, 3 * part_len, rng.randrange(400)))
                    for _ in range(rng.randrange(1, 40))]
            parts, long_rows, long_first = plan(lib, lens, short_max, part_len)
            rp = [0]
            for n in lens:
                rp.append(rp[-1] + n)
            assert long_rows == [r for r, n in enumerate(lens) if n > short_max]
            assert long_first[0] == 0 and long_first[-1] == len(parts) and len(long_first) == len(long_rows) + 1
            for k, r in enumerate(long_rows):
                mine = parts[long_first[k]:long_first[k + 1]]
                assert mine and all(p[0] == r for p in mine)
                at = rp[r]
                for _, first, n in mine:
                    assert first == at and 1 <= n <= part_len
                    at += n
                assert at == rp[r + 1]
                assert all(n == part_len for _, _, n in mine[:-1])
            assert {p[0] for p in parts} == set(long_rows)             # no short row has a part


# ---------------------------------------------------------------------------------------------- the CSR rule

def check(lib, rp, col, rows, cols, nnz):
    pos, val, msg = C.c_uint64(), C.c_uint32(), C.create_string_buffer(200)
    kind = lib.spmv_check(u32(rp), u32(col), rows, cols, nnz, C.byref(pos), C.byref(val), msg, 200)
    return kind, pos.value, val.value, msg.value.decode()


GOOD_RP, GOOD_COL = [0, 2, 2, 5, 6], [3, 0, 1, 1, 4, 2]   # 4 x 5, 6 entries, an empty row, a repeated column


def test_a_sound_matrix_passes_and_each_defect_alone_is_named(lib):
    assert check(lib, GOOD_RP, GOOD_COL, 4, 5, 6) == (0, 0, 0, "")
    assert check(lib, [0], [], 0, 0, 0)[0] == 0 and check(lib, [0, 0, 0], [], 2, 7, 0)[0] == 0
    assert check(lib, [1, 2, 2, 5, 6], GOOD_COL, 4, 5, 6) == (1, 0, 1, "row_ptr[0] = 1 but must be 0")
    kind, pos, val, msg = check(lib, [0, 2, 1, 5, 6], GOOD_COL, 4, 5, 6)
    assert (kind, pos, val) == (1, 2, 1) and msg.startswith("row_ptr[2] = 1 but row_ptr[1] = 2")
    kind, pos, val, msg = check(lib, [0, 2, 2, 5, 7], GOOD_COL + [0], 4, 5, 6)
    assert (kind, pos, val) == (1, 4, 7) and msg.startswith("row_ptr[4] = 7 but nnz = 6")
    kind, pos, val, msg = check(lib, [0, 2, 2, 5, 5], GOOD_COL, 4, 5, 6)
    assert (kind, pos, val) == (1, 4, 5) and msg.startswith("row_ptr[4] = 5 but nnz = 6")
    assert check(lib, GOOD_RP, [3, 0, 1, 5, 4, 2], 4, 5, 6) == (2, 3, 5, "col[3] = 5 but cols = 5")
    assert check(lib, GOOD_RP, [3, 0, 1, 1, 4, 0xFFFFFFFF], 4, 5, 6) == (2, 5, 0xFFFFFFFF, "col[5] = 4294967295 but cols = 5")
    assert check(lib, [7], [], 0, 0, 0)[:3] == (1, 0, 7)           # no rows: the one word is both the first and the last


def test_the_smallest_defect_is_reported_and_row_ptr_comes_first(lib):
    kind, pos, val, _ = check(lib, [0, 3, 2, 1, 6], GOOD_COL, 4, 5, 6)
    assert (kind, pos, val) == (1, 2, 2)
    assert check(lib, GOOD_RP, [9, 0, 8, 1, 7, 2], 4, 5, 6)[:3] == (2, 0, 9)
    # a bad column at position 0 and a bad row_ptr at its end: the row_ptr defect is the one named, and col was never read
    assert check(lib, [0, 2, 2, 5, 9], [9, 9, 9, 9, 9, 9], 4, 5, 6)[:3] == (1, 4, 9)
    # the rule entry by entry, as a lane applies it
    assert lib.spmv_row_ptr_entry_ok(0, 12345, 0, 4, 6) == 1 and lib.spmv_row_ptr_entry_ok(0, 0, 1, 4, 6) == 0
    assert lib.spmv_row_ptr_entry_ok(2, 2, 2, 4, 6) == 1 and lib.spmv_row_ptr_entry_ok(2, 3, 2, 4, 6) == 0
    assert lib.spmv_row_ptr_entry_ok(4, 5, 6, 4, 6) == 1 and lib.spmv_row_ptr_entry_ok(4, 5, 7, 4, 6) == 0
    assert lib.spmv_col_entry_ok(4, 5) == 1 and lib.spmv_col_entry_ok(5, 5) == 0 and lib.spmv_col_entry_ok(0, 0) == 0


# ---------------------------------------------------------------------------------------------- the transposition

def transpose_model(rows, cols, rp, col, val):
    """stable: entries of a transposed row in the order of the original rows, and of the entries inside a row"""
    by_col = [[] for _ in range(cols)]
    for r in range(rows):
        for j in range(rp[r], rp[r + 1]):
            by_col[col[j]].append((r, None if val is None else val[j]))
    t_rp = [0]
    for c in by_col:
        t_rp.append(t_rp[-1] + len(c))
    flat = [e for c in by_col for e in c]
    return t_rp, [e[0] for e in flat], None if val is None else [e[1] for e in flat]


def transpose(lib, rows, cols, rp, col, val):
    nnz = len(col)
    t_rp, t_col, t_val = (C.c_uint32 * (cols + 1))(), (C.c_uint32 * max(nnz, 1))(), (C.c_uint32 * (8 * max(nnz, 1)))()
    lib.spmv_transpose(rows, cols, nnz, u32(rp), u32(col), None if val is None else vec(val), t_rp, t_col, None if val is None else t_val)
    return list(t_rp), list(t_col[:nnz]), None if val is None else [value(t_val, j) for j in range(nnz)]


def test_the_host_transposition_against_the_model(lib):
    rng = random.Random("spmv/transpose")
    # stability and duplicates: row 0 names column 2 twice, with different values, between other columns; column 3 is empty
    rp, col, val = [0, 4, 4, 6], [2, 0, 2, 1, 2, 0], [10, 11, 12, 13, 14, 15]
    assert transpose(lib, 3, 5, rp, col, val) == ([0, 2, 3, 6, 6, 6], [0, 2, 0, 0, 0, 2], [11, 15, 13, 10, 12, 14])
    assert transpose(lib, 3, 5, rp, col, val) == transpose_model(3, 5, rp, col, val)
    assert transpose(lib, 3, 5, rp, col, None) == transpose_model(3, 5, rp, col, None)
    # a column hit by every row, empty columns, empty rows
    for rows, cols in ((1, 1), (7, 3), (40, 9), (5, 60)):
        rp, col = [0], []
        for r in range(rows):
            mine = [0] + [rng.randrange(cols) for _ in range(rng.choice((0, 0, 1, 3, 8)))]
            rng.shuffle(mine)
            col += mine
            rp.append(len(col))
        val = [rng.randrange(1 << 256) for _ in col]
        got = transpose(lib, rows, cols, rp, col, val)
        assert got == transpose_model(rows, cols, rp, col, val)
        assert got[0][1] - got[0][0] >= rows and got[1][:got[0][1]] == sorted(got[1][:got[0][1]])
    assert transpose(lib, 0, 4, [0], [], None) == ([0, 0, 0, 0, 0], [], None)
    assert transpose(lib, 3, 0, [0, 0, 0, 0], [], []) == ([0], [], [])
