"""The lane bodies of montgomery_amd/csrc/scalar_vec.h on the CPU (tests/csrc/scalars_host.hip), over the scalar field the
dispatch gives each of the seven curves, bit for bit against Python integers mod cv.q.

Elements are raw 256-bit integers -- an element >= q stands for its residue -- and every result must be canonical.  The edge
operands (0, 1, q - 1, q, q + 1, 2^256 - 1) drive the value bounds written in the header of scalar_vec.h to their ends: the
largest raw products, on the 251-bit modulus of Ed-on-BLS12-377 as on the 255-bit ones."""
import ctypes as C
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

from host_lib import host_library, value, words  # noqa: E402

TOP = (1 << 256) - 1


@pytest.fixture(scope="module")
def lib():
    L = host_library("scalars_host")
    u32p = C.POINTER(C.c_uint32)
    L.sv_modulus.argtypes = [C.c_int, u32p]
    L.sv_lincomb.argtypes = [C.c_int, u32p, u32p, u32p, u32p, u32p]
    L.sv_mul.argtypes = [C.c_int, u32p, u32p, u32p]
    L.sv_powers.argtypes = [C.c_int, u32p, u32p, u32p, C.c_int, u32p]
    L.sv_inner.argtypes = [C.c_int, u32p, u32p, C.c_int, C.c_int, u32p]
    L.sv_combine.argtypes = [C.c_int, u32p, u32p, u32p]
    return L


def vec(vals):   # not host_lib.vec: an empty list gives an empty array here, not one spare element
    return (C.c_uint32 * (8 * len(vals)))(*[(v >> (32 * j)) & 0xFFFFFFFF for v in vals for j in range(8)])


def operands(cv, tag):
    """the edge elements and 64 random ones, below 2^256 (not reduced: the top ones exceed q)"""
    q = cv.q
    return [0, 1, q - 1, q, q + 1, TOP] + O.prng_ints(f"scalars/host/{tag}/{cv.name}", 64, 1 << 256)


def host_scalars(cv, tag):
    q = cv.q
    return [0, 1, q - 1, O.prng_ints(f"scalars/host/{tag}/x/{cv.name}", 1, q)[0]]


@pytest.mark.parametrize("name", D.NAMES)
def test_dispatched_field_is_the_group_order(lib, name):
    cv = D.CURVE_TABLE[name]
    out = (C.c_uint32 * 8)()
    assert lib.sv_modulus(cv.cid, out) == 0
    assert value(out) == cv.q
    assert lib.sv_modulus(99, out) == -1


@pytest.mark.parametrize("name", D.NAMES)
def test_lincomb_lane(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    A, B = operands(cv, "lc/a"), operands(cv, "lc/b")
    B = B[3:] + B[:3]                                    # every edge value of a meets another one of b
    out = (C.c_uint32 * 8)()
    for x in host_scalars(cv, "lc"):
        for y in host_scalars(cv, "lc2"):
            for a, b in zip(A, B):
                assert lib.sv_lincomb(cv.cid, words(x), words(a), words(y), words(b), out) == 0
                assert value(out) == (x * a + y * b) % q, (name, x, y, a, b)
        for a in A:
            assert lib.sv_lincomb(cv.cid, words(x), words(a), None, None, out) == 0
            assert value(out) == x * a % q, (name, x, a)
    # the extreme of the bound: both terms the largest raw element under the largest scalar
    assert lib.sv_lincomb(cv.cid, words(q - 1), words(TOP), words(q - 1), words(TOP), out) == 0
    assert value(out) == 2 * (q - 1) * TOP % q


@pytest.mark.parametrize("name", D.NAMES)
def test_mul_lane(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    A, B = operands(cv, "mul/a"), operands(cv, "mul/b")
    out = (C.c_uint32 * 8)()
    edge = A[:6]
    pairs = [(a, b) for a in edge for b in edge] + list(zip(A[6:], B[6:]))
    for a, b in pairs:
        assert lib.sv_mul(cv.cid, words(a), words(b), out) == 0
        assert value(out) == a * b % q, (name, a, b)


@pytest.mark.parametrize("name", D.NAMES)
def test_powers_lane(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    idx = sorted({0, 1, 63, 64} | {(1 << k) - 1 for k in range(30)} | {1 << k for k in range(30)} | {(1 << 30) - 1})
    ibuf = (C.c_uint32 * len(idx))(*idx)
    out = (C.c_uint32 * (8 * len(idx)))()
    r = O.prng_ints(f"scalars/host/pow/{name}", 2, q)
    for s, x in ((1, r[0]), (r[1], r[0]), (q - 1, q - 1), (r[1], 0), (r[1], 1), (0, r[0]), (1, 2)):
        assert lib.sv_powers(cv.cid, words(s), words(x), ibuf, len(idx), out) == 0
        for t, i in enumerate(idx):
            assert value(out, t) == s * pow(x, i, q) % q, (name, s, x, i)


@pytest.mark.parametrize("name", D.NAMES)
def test_inner_terms_combine_and_finish(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    A, B = operands(cv, "in/a"), operands(cv, "in/b")
    edge = A[:6]
    out = (C.c_uint32 * 8)()
    # two terms over every pair of edge products: term, combine, finish
    for a0 in edge:
        for b0 in edge:
            for a1, b1 in ((TOP, TOP), (q - 1, q - 1), (0, 1), (q, q + 1)):
                assert lib.sv_inner(cv.cid, vec([a0, a1]), vec([b0, b1]), 2, 1, out) == 0
                assert value(out) == (a0 * b0 + a1 * b1) % q, (name, a0, b0, a1, b1)
    # a longer sum, cut into two accumulators at several places: the same bits wherever it is cut
    n = len(A)
    exp = sum(a * b for a, b in zip(A, B)) % q
    for cut in (0, 1, 6, n // 2, n):
        assert lib.sv_inner(cv.cid, vec(A), vec(B), n, cut, out) == 0
        assert value(out) == exp, (name, cut)
    # the all-maximal sum: 70 terms of (2^256 - 1)^2
    assert lib.sv_inner(cv.cid, vec([TOP] * 70), vec([TOP] * 70), 70, 35, out) == 0
    assert value(out) == 70 * TOP * TOP % q
    assert lib.sv_inner(cv.cid, vec([]), vec([]), 0, 0, out) == 0 and value(out) == 0


@pytest.mark.parametrize("name", D.NAMES)
def test_combine_step_keeps_its_invariant(lib, name):
    """acc, t < 2 q in, acc + t (mod q) below 2 q out -- on the ends of the range"""
    cv = D.CURVE_TABLE[name]
    q = cv.q
    ends = [0, 1, q - 1, q, q + 1, 2 * q - 1] + [v for v in O.prng_ints(f"scalars/host/comb/{name}", 8, 2 * q)]
    out = (C.c_uint32 * 8)()
    for u in ends:
        for v in ends:
            assert lib.sv_combine(cv.cid, words(u), words(v), out) == 0
            got = value(out)
            assert got < 2 * q and (got - u - v) % q == 0, (name, u, v)
            assert got == (u + v if u + v < 2 * q else u + v - 2 * q)
