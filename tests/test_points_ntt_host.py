"""msm_points_ntt on the CPU: the index maps and the butterfly lane of montgomery_amd/csrc/points_ntt.h compiled for the host
(tests/csrc/points_ntt_host.hip).

(i)   the index maps against plain Python for every log2n <= 12 and every stage: the bit reversal is an involution that reverses
      the bits; the lane -> (j, block) map covers every row of a stage exactly once, pairs rows m / 2 apart in one block and reads
      the twiddle omega^(j n / m) at stride n / m; lanes t < n / m are the butterflies with w = 1; the count of the others over a
      transform is (n / 2)(log2n - 2) + 1;
(ii)  a radix-2 transform run through these maps in Python integers is the transform msm_points_ntt documents;
(iii) the butterfly lane bit for bit against the rows of A + w B and A - w B from the oracle, on the five curves whose scalar
      field has transforms of more than two points: generic rows under the edge twiddles 1, q - 1, lambda, q - lambda and the
      edge scalars of tests/test_points_mul_host.py, and every degenerate pairing (A or B the identity, both, A = w B, A = -w B),
      over table slots that are reused.
"""
import ctypes as C
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402
from test_points_mul_host import edge_scalars, make_row, new_table, wire_row, words  # noqa: E402

from host_lib import host_library  # noqa: E402

TWO_ADIC = ("bls377", "bls381", "pallas", "bn254", "vesta")
MAX_LOG = 12


@pytest.fixture(scope="module")
def lib():
    L = host_library("points_ntt_host")
    u32p = C.POINTER(C.c_uint32)
    L.pn_bit_reverse.argtypes = [C.c_uint32, C.c_int]
    L.pn_bit_reverse.restype = C.c_uint32
    L.pn_butterfly.argtypes = [C.c_uint32, C.c_int, C.c_int, u32p]
    L.pn_butterfly.restype = None
    L.pn_multiplications.argtypes = [C.c_int]
    L.pn_multiplications.restype = C.c_uint64
    L.pn_lane.argtypes = [C.c_int, u32p, u32p, u32p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, u32p, u32p]
    return L


@pytest.fixture(scope="module")
def pm():
    """the shim of points_mul.h: it makes rows and sizes tables"""
    L = host_library("points_mul_host")
    u32p = C.POINTER(C.c_uint32)
    L.pm_table_elems.argtypes = [C.c_int, C.c_int, C.c_uint64]
    L.pm_table_elems.restype = C.c_uint64
    L.pm_make_row.argtypes = [C.c_int, u32p, u32p]
    return L


# ---------------------------------------------------------------------------------------------- the index maps

def fly(lib, t, log2n, s):
    out = (C.c_uint32 * 4)()
    lib.pn_butterfly(t, log2n, s, out)
    return tuple(out)


def test_bit_reversal(lib):
    for L in range(MAX_LOG + 1):
        n = 1 << L
        rev = [lib.pn_bit_reverse(i, L) for i in range(n)]
        assert rev == [int(format(i, f"0{L}b")[::-1], 2) if L else 0 for i in range(n)]
        assert all(rev[rev[i]] == i for i in range(n))


def test_lane_map_twiddle_index_and_stride(lib):
    for L in range(1, MAX_LOG + 1):
        n = 1 << L
        nontrivial = 0
        for s in range(1, L + 1):
            m, blocks = 1 << s, n >> s
            seen = []
            for t in range(n // 2):
                a, b, j, tw = fly(lib, t, L, s)
                assert (j, a // m) == (t // blocks, t % blocks), (L, s, t)       # lane t: position j of block t mod (n / m)
                assert a % m == j and b == a + m // 2 and j < m // 2
                assert tw == j * blocks and tw < max(n // 2, 1)                  # omega^(j n / m) of the vector omega^0 .. omega^(n/2-1)
                assert (j == 0) == (t < blocks)                                  # the butterflies with w = 1 are the first n / m lanes
                nontrivial += j != 0
                seen += [a, b]
            assert sorted(seen) == list(range(n))                                # every row of the stage, once
            if blocks >= 64:                                                     # whole waves share one position, so one twiddle
                assert all(len({fly(lib, t, L, s)[2] for t in range(w, w + 64)}) == 1 for w in range(0, n // 2, 64))
        want = (n // 2) * (L - 2) + 1 if L >= 2 else 0
        assert nontrivial == want == lib.pn_multiplications(L), L
    assert lib.pn_multiplications(0) == 0


def test_the_maps_make_the_documented_transform(lib):
    """Bit reversal, then the stages with butterflies (A, B) -> (A + w B, A - w B) through the shim's maps, over integers mod a
    small prime: D[k] = sum_j omega^(j k) A[j]."""
    p, g = 12289, 11                                                             # 12289 = 3 * 2^12 + 1, 11 generates its units
    for L in range(MAX_LOG + 1 - 4):
        n = 1 << L
        om = pow(g, (p - 1) >> L, p)
        a = [(7 * i * i + 3 * i + 1) % p for i in range(n)]
        d = [a[lib.pn_bit_reverse(i, L)] for i in range(n)]
        tws = [pow(om, j, p) for j in range(max(n // 2, 1))]
        for s in range(1, L + 1):
            for t in range(n // 2):
                ia, ib, j, tw = fly(lib, t, L, s)
                wb = tws[tw] * d[ib] % p
                d[ia], d[ib] = (d[ia] + wb) % p, (d[ia] - wb) % p
        assert d == [sum(a[j] * pow(om, j * k, p) for j in range(n)) % p for k in range(n)], L


# ---------------------------------------------------------------------------------------------- the butterfly lane

def butterfly(lib, pm, cv, A, B, w, tbl, cap=1, g=0):
    """(row of A + w B, row of A - w B) from the lane; w = None: the lane without a multiplication"""
    rw = pm.pm_row_words(cv.cid)
    out_a, out_b = (C.c_uint32 * rw)(), (C.c_uint32 * rw)()
    tw = None if w is None else words(w, 8)
    assert lib.pn_lane(cv.cid, make_row(pm, cv, A), make_row(pm, cv, B), tw, int(w is not None), None if w is None else tbl, cap, g,
                       out_a, out_b) == 0
    return list(out_a), list(out_b)


def expected(cv, A, B, w):
    wB = None if B is None or w % cv.q == 0 else cv.scale(w % cv.q, B)
    return wire_row(cv, cv.add(A, wB)), wire_row(cv, cv.add(A, cv.neg(wB)))


@pytest.mark.parametrize("name", TWO_ADIC)
def test_generic_rows_under_edge_twiddles(lib, pm, name):
    """Every lane runs over the same table slots, lane 1 of 3, with other rows each time: no stale entry survives."""
    cv = D.CURVE_TABLE[name]
    pts = D.pool(name)[0]
    q, lam = cv.q, cv.B.lam
    tbl = new_table(pm, cv, pm.pm_built_w(), 3)
    tw = [1, q - 1, lam, q - lam] + edge_scalars(cv) + O.prng_ints(f"points_ntt/lane/{name}", 4, q)
    for i, w in enumerate(dict.fromkeys(tw)):
        A, B = pts[i % D.POOL], pts[(5 * i + 1) % D.POOL]
        assert butterfly(lib, pm, cv, A, B, w, tbl, 3, 1) == expected(cv, A, B, w), (name, hex(w))
    n, step = len(tbl), 4 * 3                                                    # the neighbours' slots were never written
    assert all(tbl[j] == 0xA5A5A5A5 for j in range(0, n, step)) and all(tbl[j] == 0xA5A5A5A5 for j in range(8, n, step))
    assert any(tbl[j] != 0xA5A5A5A5 for j in range(4, n, step))
    for i in range(4):                                                           # w = 1 without the multiplication
        A, B = pts[i], pts[i + 9]
        assert butterfly(lib, pm, cv, A, B, None, None) == expected(cv, A, B, 1), (name, i)


@pytest.mark.parametrize("name", TWO_ADIC)
def test_every_degenerate_pairing(lib, pm, name):
    cv = D.CURVE_TABLE[name]
    pts = D.pool(name)[0]
    q = cv.q
    tbl = new_table(pm, cv, pm.pm_built_w(), 1)
    P, Q = pts[3], pts[11]
    for w in (None, 1, q - 1, cv.B.lam, O.prng_ints(f"points_ntt/deg/{name}", 1, q)[0] | 2):
        ww = 1 if w is None else w
        wQ = cv.scale(ww, Q)
        pairs = [(None, Q), (P, None), (None, None), (wQ, Q), (cv.neg(wQ), Q), (P, Q)]
        for A, B in pairs:
            got = butterfly(lib, pm, cv, A, B, w, tbl)
            assert got == expected(cv, A, B, ww), (name, w, A is None, B is None)
        ident = wire_row(cv, None)
        assert butterfly(lib, pm, cv, None, None, w, tbl) == (ident, ident)
        assert butterfly(lib, pm, cv, cv.neg(wQ), Q, w, tbl)[0] == ident         # A + w B cancels
        assert butterfly(lib, pm, cv, wQ, Q, w, tbl)[1] == ident                 # A - w B cancels, A + w B doubles
        assert butterfly(lib, pm, cv, wQ, Q, w, tbl)[0] == wire_row(cv, cv.add(wQ, wQ))
    # a twiddle of 0 (no transform has one; the walk gives the identity): both rows are A
    assert butterfly(lib, pm, cv, P, Q, 0, tbl) == (wire_row(cv, P), wire_row(cv, P))
