"""The plan, the combine operators and the inverse lane body of montgomery_amd/csrc/scalar_scan.h on the CPU
(tests/csrc/scans_host.hip), against Python integers mod q, on the scalar fields of all seven curves.

The plan is checked against levels derived by hand.  The operators take both operands from {0, 1, q - 1, q, q + 1, 2^256 - 1}, the
ends of the value bounds in the header of scalar_scan.h, in every pairing; the result must be canonical.  The inverse walks chains
that hold multiples of q (0, q, 2 q and the largest one below 2^256) in the first, a middle, the last and every position."""
import ctypes as C
import itertools
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

from host_lib import host_library, value, words  # noqa: E402

TOP = (1 << 256) - 1
SUM, PRODUCT, HORNER = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    L = host_library("scans_host")
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    L.scans_plan.argtypes = [C.c_uint64, C.c_int, i32p]
    L.scans_modulus.argtypes = [C.c_int, u32p]
    L.scans_combine.argtypes = [C.c_int, C.c_int, u32p, u32p, u32p, C.c_int, u32p]
    L.scans_inverse.argtypes = [C.c_int, u32p, C.c_uint64, C.c_uint32, u32p, C.POINTER(C.c_uint64)]
    return L


def vec(vals):   # not host_lib.vec: an empty list gives an empty array here, not one spare element
    return (C.c_uint32 * (8 * len(vals)))(*[(v >> (32 * j)) & 0xFFFFFFFF for v in vals for j in range(8)])


def test_tile_constants(lib):
    assert lib.scans_block() == 256 and lib.scans_min_tile_log() == 8        # tile_log 8: one element per lane
    assert lib.scans_min_tile_log() <= lib.scans_default_tile_log()
    assert 3 * lib.scans_default_tile_log() >= 30                            # at most three levels below 2^30 at the default
    assert lib.scans_inverse_e() >= 1 and lib.scans_max_levels() == 4


@pytest.mark.parametrize("name", D.NAMES)
def test_dispatched_field_is_the_group_order(lib, name):
    cv = D.CURVE_TABLE[name]
    out = (C.c_uint32 * 8)()
    assert lib.scans_modulus(cv.cid, out) == 0 and value(out) == cv.q
    assert lib.scans_modulus(99, out) == -1


def test_plan_against_hand_derived_levels(lib):
    out = (C.c_int32 * 4)()

    def plan(n, tile_log):
        return list(out[:lib.scans_plan(n, tile_log, out)])

    for tile_log in range(lib.scans_min_tile_log(), lib.scans_default_tile_log() + 1):
        T = 1 << tile_log
        assert plan(0, tile_log) == []
        assert plan(1, tile_log) == [1]
        assert plan(T - 1, tile_log) == [1]
        assert plan(T, tile_log) == [1]
        assert plan(T + 1, tile_log) == [2, 1]
        assert plan(T * T - 1, tile_log) == [T, 1]
        assert plan(T * T, tile_log) == [T, 1]
        assert plan(T * T + 1, tile_log) == [T + 1, 2, 1]
    # 2^30 - 1 elements: 2^22, 2^14, 2^6 tiles and the top at 2^8; 2^21, 2^12, 2^3, 1 at 2^9; three levels at 2^10
    assert plan((1 << 30) - 1, 8) == [1 << 22, 1 << 14, 1 << 6, 1]
    assert plan((1 << 30) - 1, 9) == [1 << 21, 1 << 12, 1 << 3, 1]
    assert plan((1 << 30) - 1, 10) == [1 << 20, 1 << 10, 1]
    # every level is the number of tiles over the level below, and the last has one tile
    for tile_log in (8, 9, 10):
        for n in (2, 255, 257, 1000, 65537, 1 << 20, (1 << 24) + 3):
            levels, m = plan(n, tile_log), n
            for t in levels:
                assert t == -(-m >> tile_log)
                m = t
            assert levels[-1] == 1


@pytest.mark.parametrize("name", D.NAMES)
def test_operators_at_the_ends_of_the_bounds(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    edge = (0, 1, q - 1, q, q + 1, TOP)
    zs = (0, 1, q - 1, O.prng_ints(f"scans/host/z/{name}", 1, q)[0])
    out = (C.c_uint32 * 8)()
    for a, b in itertools.product(edge, edge):
        assert lib.scans_combine(cv.cid, SUM, words(a), words(b), words(0), 0, out) == 0
        assert value(out) == (a + b) % q, (name, "sum", a, b)
        assert lib.scans_combine(cv.cid, PRODUCT, words(a), words(b), words(0), 0, out) == 0
        assert value(out) == a * b % q, (name, "product", a, b)
        for z in zs:
            for k in (0, 1, 5, 13, 39):
                assert lib.scans_combine(cv.cid, HORNER, words(a), words(b), words(z), k, out) == 0
                assert value(out) == (a * pow(z, 1 << k, q) + b) % q, (name, "horner", a, b, z, k)


def check_inverse(lib, cv, vals, lanes):
    q, n = cv.q, len(vals)
    out, zeros = (C.c_uint32 * (8 * n))(), C.c_uint64(77)
    assert lib.scans_inverse(cv.cid, vec(vals), n, lanes, out, C.byref(zeros)) == 0
    got = [value(out, i) for i in range(n)]
    assert got == [pow(v % q, q - 2, q) for v in vals]          # 0^(q-2) = 0: a residue of 0 gives 0
    assert zeros.value == sum(1 for v in vals if v % q == 0)


@pytest.mark.parametrize("name", D.NAMES)
def test_inverse_chains_with_multiples_of_q(lib, name):
    cv = D.CURVE_TABLE[name]
    q, E = cv.q, lib.scans_inverse_e()
    multiples = (0, q, 2 * q, (TOP // q) * q)
    base = O.prng_ints(f"scans/host/inv/{name}", E, 1 << 256)
    base[1 % E] = q + 1
    base[E - 2] = TOP
    check_inverse(lib, cv, base, 1)
    check_inverse(lib, cv, [1] * E, 1)
    for m in multiples:
        for pos in (0, E // 2, E - 1):
            vals = list(base)
            vals[pos] = m
            check_inverse(lib, cv, vals, 1)
        check_inverse(lib, cv, [m] * E, 1)                      # every position
    check_inverse(lib, cv, [multiples[i % 4] for i in range(E)], 1)
    # shorter chains (a ragged last lane), and the strided walk of the kernel: 3 lanes over 2 E + 5 elements
    for n in (1, 2, E - 1):
        check_inverse(lib, cv, base[:n], 1)
        check_inverse(lib, cv, [q] + base[1:n], 1)
    long = O.prng_ints(f"scans/host/inv/long/{name}", 2 * E + 5, 1 << 256)
    long[0], long[E], long[-1] = 0, 2 * q, q
    check_inverse(lib, cv, long, 3)
