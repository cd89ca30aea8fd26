"""msm_points_lincomb on the CPU: the host recoder and the lane bodies of montgomery_amd/csrc/points_lincomb.h compiled for the
host (tests/csrc/lincomb_host.hip), on all seven curves.

(i)  the program conditions: what a program computes (its ops interpreted over integers mod q), its doublings and additions,
     the shortcuts for 0, 1 and q - 1, the empty program of a copy;
(ii) the lane body over pool points and identity rows, bit for bit against the row of cv.add(cv.scale(a, A), cv.scale(b, B)).
"""
import ctypes as C
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

from host_lib import host_library, words  # noqa: E402

OP_DBL, OP_ADD = 0, 1


@pytest.fixture(scope="module")
def lib():
    L = host_library("lincomb_host")
    u32p = C.POINTER(C.c_uint32)
    L.lc_program.argtypes = [C.c_int, u32p, u32p, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]
    L.lc_make_row.argtypes = [C.c_int, u32p, u32p, C.c_int, u32p]
    L.lc_lane.argtypes = [C.c_int, u32p, u32p, C.POINTER(C.c_uint8), C.c_int, u32p]
    return L


def program(lib, cv, a, b):
    """(ops, doublings, additions, copy) of the program of (a, b); b None: no second term."""
    ops = (C.c_uint8 * lib.lc_max_ops())()
    info = (C.c_int32 * 4)()
    assert lib.lc_program(cv.cid, words(a, 8), None if b is None else words(b, 8), ops, info) == 0
    n, n_dbl, n_add, copy = info
    got = list(ops[:n])
    assert n_dbl == got.count(OP_DBL) and n_add == n - n_dbl
    return got, n_dbl, n_add, bool(copy)


def lam_of(cv):
    return None if cv.te else cv.B.lam


def coefficients(cv, ops):
    """The integer multiples of (A, phi(A), B, phi(B)) a program accumulates."""
    acc = [0, 0, 0, 0]
    for op in ops:
        if op == OP_DBL:
            acc = [2 * v for v in acc]
        else:
            sel = op - OP_ADD
            assert 0 <= sel < 8
            acc[sel >> 1] += -1 if sel & 1 else 1
    return acc


def check_program(lib, cv, a, b):
    """The program computes a * A + b * B, within the conditions the design sets; returns (doublings, additions)."""
    ops, n_dbl, n_add, copy = program(lib, cv, a, b)
    q = cv.q
    if copy:
        assert ops == [] and a == 1 and not b
        return 0, 0
    cA, cpA, cB, cpB = coefficients(cv, ops)
    if cv.te:
        assert cpA == 0 and cpB == 0
        assert cA == (-1 if a == q - 1 else a)        # the scalars as they are: no reduction on a curve with a cofactor
        assert cB == (-1 if b == q - 1 else (b or 0))
        assert n_dbl <= 251
    else:
        lam = cv.B.lam
        assert (cA + lam * cpA - a) % q == 0 and (cB + lam * cpB - (b or 0)) % q == 0
        assert n_dbl <= lib.lc_max_bits(cv.cid) + 1
        assert max(abs(v) for v in (cA, cpA, cB, cpB)) < 1 << (lib.lc_max_bits(cv.cid) + 1)
    return n_dbl, n_add


@pytest.mark.parametrize("name", D.NAMES)
def test_programs_of_random_scalar_pairs(lib, name):
    cv = D.CURVE_TABLE[name]
    sc = O.prng_ints(f"lincomb/program/{name}", 2000, cv.q)
    worst = 0
    for a, b in zip(sc[:1000], sc[1000:]):
        n_dbl, n_add = check_program(lib, cv, a, b)
        worst = max(worst, n_dbl)
        terms = 2 if cv.te else 4
        assert n_add <= terms * ((251 if cv.te else lib.lc_max_bits(cv.cid)) // 2 + 1)   # a NAF has no two adjacent digits
    for a in sc[:50]:
        check_program(lib, cv, a, None)
    print(name, "most doublings", worst)


@pytest.mark.parametrize("name", D.NAMES)
def test_programs_of_small_and_top_scalars(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    special = (0, 1, 2, 3, q - 2, q - 1)
    for a in special:
        for b in special + (None,):
            check_program(lib, cv, a, b)
    # the copy: an empty program
    for b in (None, 0):
        assert program(lib, cv, 1, b) == ([], 0, 0, True)
    assert program(lib, cv, 0, 0) == ([], 0, 0, False) and program(lib, cv, 0, None) == ([], 0, 0, False)
    # 0, 1 and q - 1 add no doubling and at most one addition to the program of the other scalar
    for s in (2, 3, q - 2, O.prng_ints(f"lincomb/special/{name}", 1, q)[0]):
        _, dbl0, add0, _ = program(lib, cv, s, None)
        for t, extra in ((0, 0), (1, 1), (q - 1, 1)):
            for a, b in ((s, t), (t, s)):
                _, n_dbl, n_add, _ = program(lib, cv, a, b)
                assert (n_dbl, n_add) == (dbl0, add0 + extra), (a, b)
    assert program(lib, cv, 1, 1)[1:3] == (0, 2) and program(lib, cv, q - 1, None)[1:3] == (0, 1)
    assert program(lib, cv, 1, q - 1)[1:3] == (0, 2)


# ---------------------------------------------------------------------------------------------- the lane body

def make_row(lib, cv, P):
    nw, rw = lib.lc_coord_words(cv.cid), lib.lc_row_words(cv.cid)
    row = (C.c_uint32 * rw)()
    ident = P is None
    x, y = (0, 0) if ident else P
    assert lib.lc_make_row(cv.cid, words(x, nw), words(y, nw), int(ident), row) == 0
    return row


def lane(lib, cv, A, B, a, b):
    """The lane body over the rows of A and B under the program of (a, b) -> the output row as a list of words."""
    ops, _, _, copy = program(lib, cv, a, b)
    ra, rb = make_row(lib, cv, A), make_row(lib, cv, B)
    if copy:
        return list(ra)                                    # the host moves the rows of a copy: no lane runs
    out = (C.c_uint32 * lib.lc_row_words(cv.cid))()
    buf = (C.c_uint8 * max(len(ops), 1))(*ops)
    assert lib.lc_lane(cv.cid, ra, rb, buf, len(ops), out) == 0
    return list(out)


def lane_cases(cv):
    """(A, B, a, b): generic pairs, B = +-A, identities, a + b = q and a = b on one point, the shortcuts."""
    q = cv.q
    pts = D.pool(cv.name)[0]
    s = [v or 1 for v in O.prng_ints(f"lincomb/lane/{cv.name}", 8, q)]
    P0, P1, P2, Z = pts[0], pts[1], pts[2], cv.zero
    return [
        (P0, P1, s[0], s[1]), (P1, P2, s[2], s[3]),          # generic
        (P0, P0, s[0], s[1]), (P0, cv.neg(P0), s[0], s[1]),  # B = A, B = -A
        (P0, P0, s[4], q - s[4]),                            # a + b = q over one point: the sum is the identity
        (P0, cv.neg(P0), s[4], s[4]),                        # the same through B = -A
        (P0, P0, s[5], s[5]),                                # a = b over one point: every addition of a B term meets acc = +-addend
        (Z, P1, s[0], s[1]), (P0, Z, s[0], s[1]), (Z, Z, s[0], s[1]),
        (P0, P1, 1, 1), (P0, P0, 1, 1), (P0, P0, 1, q - 1), (P0, P1, q - 1, 1), (P0, P1, 0, s[6]), (P0, P1, s[7], 0),
        (P0, P1, 0, 0), (P0, P1, 1, 0), (P0, P1, 2, 0), (P0, P1, 3, 1), (P0, P1, 2, q - 2),
    ]


@pytest.mark.parametrize("name", D.NAMES)
def test_lane_body_equals_the_oracle_bit_for_bit(lib, name):
    cv = D.CURVE_TABLE[name]
    for A, B, a, b in lane_cases(cv):
        sa = cv.zero if A == cv.zero else cv.scale(a, A)
        sb = cv.zero if B == cv.zero else cv.scale(b, B)
        if cv.te:
            exp = cv.add(sa, sb)
        else:
            exp = sb if sa is None else sa if sb is None else cv.add(sa, sb)
        got = lane(lib, cv, A, B, a, b)
        assert got == list(make_row(lib, cv, exp)), (name, a, b, A == B)


@pytest.mark.parametrize("name", D.NAMES)
def test_lane_body_without_a_second_term(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    P = D.pool(name)[0][3]
    s = O.prng_ints(f"lincomb/lane1/{name}", 1, q)[0]
    for a in (s, q - 1, 2, q - 2):
        ops, _, _, _ = program(lib, cv, a, None)
        ra = make_row(lib, cv, P)
        out = (C.c_uint32 * lib.lc_row_words(cv.cid))()
        assert lib.lc_lane(cv.cid, ra, ra, (C.c_uint8 * len(ops))(*ops), len(ops), out) == 0
        assert list(out) == list(make_row(lib, cv, cv.scale(a, P)))
