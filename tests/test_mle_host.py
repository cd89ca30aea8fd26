"""The index maps, the lane bodies and the half-table split of montgomery_amd/csrc/scalar_mle.h on the CPU
(tests/csrc/mle_host.hip), over the scalar field the dispatch gives each of the seven curves, bit for bit against Python integers
mod cv.q.

Elements are raw 256-bit integers -- an element >= q stands for its residue -- and every result must be canonical.  The edge
operands (0, 1, q - 1, q, q + 1, 2^256 - 1) in every pairing of (lo, hi) drive the value bounds written in the header of
scalar_mle.h to their ends: the largest raw difference, the largest stepped value lo + d (hi - lo + M q) at t = d, on the 251-bit
modulus of Ed-on-BLS12-377 as on the 255-bit ones."""
import ctypes as C
import itertools
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

from host_lib import host_library, value, vec, words  # noqa: E402
from operator_fixture import TOP, edges  # noqa: E402

PROD, R1CS = 0, 1
SHAPES = [(PROD, 1), (PROD, 2), (PROD, 3), (PROD, 4), (R1CS, 4)]


@pytest.fixture(scope="module")
def lib():
    L = host_library("mle_host")
    u32p = C.POINTER(C.c_uint32)
    L.mle_pair_lo.argtypes = L.mle_pair_hi.argtypes = [C.c_uint64, C.c_uint32]
    L.mle_pair_lo.restype = L.mle_pair_hi.restype = C.c_uint64
    L.mle_round_values.argtypes = L.mle_round_owed.argtypes = [C.c_int, C.c_int]
    L.mle_eq_split.argtypes = [C.c_uint32]
    L.mle_constants.argtypes = [C.c_int, u32p]
    L.mle_round.argtypes = [C.c_int, C.c_int, C.c_int, u32p, C.c_int, C.c_int, C.c_int, u32p]
    L.mle_finish.argtypes = [C.c_int, C.c_int, C.c_int, u32p, u32p]
    L.mle_reduce_wide.argtypes = [C.c_int, u32p, u32p]
    L.mle_bind.argtypes = [C.c_int, u32p, u32p, u32p, u32p]
    L.mle_eq.argtypes = [C.c_int, u32p, C.c_uint32, u32p, u32p, u32p]
    return L


def g_of(shape, f, q):
    if shape == R1CS:
        return f[0] * (f[1] * f[2] - f[3]) % q
    p = 1
    for x in f:
        p = p * x % q
    return p


def expected_round(shape, m, pairs, q):
    """pairs: per vector a list of (lo, hi); -> s(0 .. d)"""
    d = 3 if shape == R1CS else m
    n_pairs = len(pairs[0])
    return [sum(g_of(shape, [pairs[j][p][0] + t * (pairs[j][p][1] - pairs[j][p][0]) for j in range(m)], q) for p in range(n_pairs)) % q
            for t in range(d + 1)]


def flat(pairs):
    return vec([x for per_vec in pairs for lo_hi in per_vec for x in lo_hi])


# ---------------------------------------------------------------------------------------------- index maps and shapes

def test_index_maps_for_every_variable_up_to_six(lib):
    for log2n in range(1, 7):
        n, h = 1 << log2n, 1 << (log2n - 1)
        for var in range(log2n):
            lo = [lib.mle_pair_lo(i, var) for i in range(h)]
            hi = [lib.mle_pair_hi(i, var) for i in range(h)]
            assert lo == [((i >> var) << (var + 1)) | (i & ((1 << var) - 1)) for i in range(h)], (log2n, var)
            assert hi == [x + (1 << var) for x in lo]
            # the pairs are the indices with bit var clear, in ascending order, and together with hi they cover the table once
            assert lo == [x for x in range(n) if not (x >> var) & 1]
            assert sorted(lo + hi) == list(range(n))
    # pair indices beyond 32 bits keep their upper bits
    assert lib.mle_pair_lo((1 << 28) - 1, 28) == (1 << 28) - 1 and lib.mle_pair_hi((1 << 28) - 1, 0) == (1 << 29) - 1
    assert lib.mle_pair_lo(1 << 33, 3) == 1 << 34


def test_values_owed_factors_and_the_split(lib):
    assert [lib.mle_round_values(s, m) for s, m in SHAPES] == [2, 3, 4, 5, 4]
    assert [lib.mle_round_owed(s, m) for s, m in SHAPES] == [0, 1, 2, 3, 2]
    assert [lib.mle_eq_split(v) for v in range(8)] == [0, 1, 1, 2, 2, 3, 3, 4]
    assert lib.mle_eq_split(29) == 15


@pytest.mark.parametrize("name", D.NAMES)
def test_field_constants(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    out = (C.c_uint32 * 10)()
    assert lib.mle_constants(cv.cid, out) == 0
    mq = sum(int(out[i]) << (30 * i) for i in range(9))
    assert all(out[i] < 1 << 30 for i in range(8))
    assert mq % q == 0 and mq >= 1 << 256 and mq - q < 1 << 256            # the smallest multiple of q at or above 2^256
    c = int(out[9])
    assert c <= (1 << 270) // q < c + 2
    assert lib.mle_constants(99, out) == -1


@pytest.mark.parametrize("name", D.NAMES)
def test_reduce_wide(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    out = (C.c_uint32 * 9)()
    vals = [0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, TOP, TOP + 1, 5 * TOP, (1 << 262) - 1, 55 * q - 1, 55 * q]
    top_k = (1 << 262) // q                                               # the largest multiple of q below 2^262 and its neighbours
    vals += [k * q + e for k in (1, 2, 31, 63, 64, top_k // 2, top_k - 1, top_k) for e in (-1, 0, 1) if k * q + e < 1 << 262]
    vals += O.prng_ints(f"mle/host/wide/{name}", 64, 1 << 262)
    for v in vals:
        assert v < 1 << 262
        assert lib.mle_reduce_wide(cv.cid, words(v, 9), out) == 0
        got = value(out, 0, 9)
        assert got < 2 * q and (got - v) % q == 0, (name, v)


# ---------------------------------------------------------------------------------------------- the round

@pytest.mark.parametrize("name", D.NAMES)
@pytest.mark.parametrize("shape,m", SHAPES)
def test_one_pair_on_the_edge_operands(lib, name, shape, m):
    """every pairing (lo, hi) of the edge operands in every vector position while the other vectors hold the largest pair, and
    every pairing in all vectors at once: the values at t = 0 .. d, t = d included"""
    cv = D.CURVE_TABLE[name]
    q = cv.q
    E = edges(q)
    out = (C.c_uint32 * 40)()
    cases = []
    for lo, hi in itertools.product(E, E):
        cases.append([[(lo, hi)]] * m)
        for pos in range(m):
            for other in ((TOP, 0), (0, TOP), (q + 1, q - 1)):
                cases.append([[(lo, hi)] if j == pos else [other] for j in range(m)])
    for pairs in cases:
        assert lib.mle_round(cv.cid, shape, m, flat(pairs), 1, 1, 1, out) == len(expected_round(shape, m, pairs, q))
        exp = expected_round(shape, m, pairs, q)
        assert [value(out, t) for t in range(len(exp))] == exp, (name, shape, m, pairs)


@pytest.mark.parametrize("name", D.NAMES)
@pytest.mark.parametrize("shape,m", SHAPES)
def test_sums_of_pairs_combine_and_finish(lib, name, shape, m):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    n_pairs = 70
    raw = O.prng_ints(f"mle/host/round/{name}/{shape}/{m}", 2 * m * n_pairs, 1 << 256)
    E = edges(q)
    for i in range(0, len(raw), 5):
        raw[i] = E[(i // 5) % 6]
    pairs = [[(raw[2 * (j * n_pairs + p)], raw[2 * (j * n_pairs + p) + 1]) for p in range(n_pairs)] for j in range(m)]
    exp = expected_round(shape, m, pairs, q)
    out = (C.c_uint32 * 40)()
    # the same bits wherever the walk is cut into two accumulator sets
    for cut in (0, 1, 35, n_pairs):
        assert lib.mle_round(cv.cid, shape, m, flat(pairs), n_pairs, cut, 1, out) == len(exp)
        assert [value(out, t) for t in range(len(exp))] == exp, (name, shape, m, cut)
    # the accumulators before the finish: below 2 q, owing R^owed with R = 2^270
    owed = lib.mle_round_owed(shape, m)
    assert lib.mle_round(cv.cid, shape, m, flat(pairs), n_pairs, 35, 0, out) == len(exp)
    for t, e in enumerate(exp):
        acc = value(out, t)
        assert acc < 2 * q and acc * pow(1 << 270, owed, q) % q == e, (name, shape, m, t)
    # 70 pairs of the largest operands
    big = [[(0, TOP)] * n_pairs] * m
    assert lib.mle_round(cv.cid, shape, m, flat(big), n_pairs, 35, 1, out) == len(exp)
    assert [value(out, t) for t in range(len(exp))] == expected_round(shape, m, big, q)
    # no pairs at all
    assert lib.mle_round(cv.cid, shape, m, vec([]), 0, 0, 1, out) == len(exp)
    assert [value(out, t) for t in range(len(exp))] == [0] * len(exp)
    assert lib.mle_round(cv.cid, shape, 5, vec([]), 0, 0, 1, out) == -1
    assert lib.mle_round(cv.cid, 2, m, vec([]), 0, 0, 1, out) == -1
    if shape == R1CS:
        assert lib.mle_round(cv.cid, R1CS, 3, vec([]), 0, 0, 1, out) == -1


@pytest.mark.parametrize("name", D.NAMES)
def test_finish_step_returns_the_factors_owed(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    R = 1 << 270
    out = (C.c_uint32 * 8)()
    accs = [0, 1, q - 1, q, q + 1, 2 * q - 1] + O.prng_ints(f"mle/host/finish/{name}", 8, 2 * q)
    for shape, m in SHAPES:
        owed = lib.mle_round_owed(shape, m)
        for acc in accs:
            assert lib.mle_finish(cv.cid, shape, m, words(acc), out) == 0
            assert value(out) == acc * pow(R, owed, q) % q, (name, shape, m, acc)


# ---------------------------------------------------------------------------------------------- bind

@pytest.mark.parametrize("name", D.NAMES)
def test_bind_lane(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    E = edges(q)
    rs = [0, 1, q - 1, 2] + O.prng_ints(f"mle/host/bind/r/{name}", 2, q)
    rnd = O.prng_ints(f"mle/host/bind/{name}", 64, 1 << 256)
    out = (C.c_uint32 * 8)()
    for r in rs:
        for lo, hi in list(itertools.product(E, E)) + list(zip(rnd[:32], rnd[32:])):
            assert lib.mle_bind(cv.cid, words(lo), words(hi), words(r), out) == 0
            assert value(out) == (lo + r * (hi - lo)) % q, (name, r, lo, hi)


# ---------------------------------------------------------------------------------------------- eq

@pytest.mark.parametrize("name", D.NAMES)
def test_eq_tables_for_zero_to_seven_variables(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    for v in range(8):
        k = (v + 1) // 2
        r = O.prng_ints(f"mle/host/eq/{name}/{v}", v, q)
        for point, s in ((r, 1), (r, q - 1), (r, O.prng_ints(f"mle/host/eq/s/{name}/{v}", 1, q)[0]),
                         ([(j * 5 + v) % 2 for j in range(v)], 1), ([q - 1] * v, 3), ([0] * v, 0)):
            out = (C.c_uint32 * (8 << v))()
            tab = (C.c_uint32 * (8 * ((1 << k) + (1 << (v - k)))))()
            assert lib.mle_eq(cv.cid, vec(point), v, words(s), out, tab) == k

            def eq(bits, first, i):
                p = 1
                for j in range(bits):
                    p = p * (point[first + j] if (i >> j) & 1 else 1 - point[first + j]) % q
                return p

            assert [value(out, i) for i in range(1 << v)] == [s * eq(v, 0, i) % q for i in range(1 << v)], (name, v, s)
            # the low half-table is plain, the high one carries s in Montgomery form (R = 2^270)
            assert [value(tab, e) for e in range(1 << k)] == [eq(k, 0, e) for e in range(1 << k)]
            assert [value(tab, (1 << k) + e) for e in range(1 << (v - k))] == \
                [s * (1 << 270) * eq(v - k, k, e) % q for e in range(1 << (v - k))]
        # a point of zeros and ones gives the indicator of its index
        bits = [(v * 3 + j) % 2 for j in range(v)]
        out = (C.c_uint32 * (8 << v))()
        assert lib.mle_eq(cv.cid, vec(bits), v, words(1), out, None) == k
        idx = sum(b << j for j, b in enumerate(bits))
        assert [value(out, i) for i in range(1 << v)] == [int(i == idx) for i in range(1 << v)]
