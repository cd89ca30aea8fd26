"""The plan, the butterfly and the whole transform of montgomery_amd/csrc/scalar_ntt.h on the CPU (tests/csrc/ntt_host.hip): the
shim's executor walks the passes, blocks, lanes and stages through the functions the kernel calls -- pass geometry, tile index
functions, twiddle exponents, lane bodies -- on an image of the LDS tile, and must give tests/ntt_model.py bit for bit.

The butterfly takes u, v from {0, 1, q - 1, q, q + 1, 2^256 - 1}: the ends of the value bounds in the header of scalar_ntt.h (a raw
element is brought below 2 q first, as the first load of a transform does; both results must be below 2 q again)."""
import ctypes as C
import itertools
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402
import ntt_model as M  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

from host_lib import host_library, value, words  # noqa: E402

TOP = (1 << 256) - 1
SCALE_NONE, SCALE_CONST, SCALE_TABLE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    L = host_library("ntt_host")
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    L.ntt_plan.argtypes = [C.c_int, C.c_int, i32p]
    L.ntt_modulus.argtypes = [C.c_int, u32p]
    L.ntt_butterfly.argtypes = [C.c_int, u32p, u32p, u32p, C.c_int, u32p, u32p]
    L.ntt_exec.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, u32p, C.c_int, u32p, u32p, C.c_int, u32p, u32p]
    return L


def vec(vals):   # not host_lib.vec: an empty list gives an empty array here, not one spare element
    return (C.c_uint32 * (8 * len(vals)))(*[(v >> (32 * j)) & 0xFFFFFFFF for v in vals for j in range(8)])


def run(lib, cv, log2n, B, tile_log, vals, omega, shift=None, inverse=False):
    """the shim's executor as msm_scalars_ntt sets a call up: omega^-1, n^-1 and shift^-1 from the host"""
    q, n = cv.q, 1 << log2n
    w = pow(omega, q - 2, q) if inverse else omega
    scale, s, x = SCALE_NONE, 0, 0
    if shift not in (None, 1) and log2n >= 1:
        scale = SCALE_TABLE
        s, x = (pow(n, q - 2, q), pow(shift, q - 2, q)) if inverse else (1, shift)
    elif inverse and log2n >= 1:
        scale, s = SCALE_CONST, pow(n, q - 2, q)
    out = (C.c_uint32 * (8 * B * n))()
    assert lib.ntt_exec(cv.cid, log2n, B, tile_log, words(w), scale, words(s), words(x), int(inverse), vec(vals), out) == 0
    return [value(out, i) for i in range(B * n)]


@pytest.mark.parametrize("name", D.NAMES)
def test_dispatched_field_is_the_group_order(lib, name):
    cv = D.CURVE_TABLE[name]
    out = (C.c_uint32 * 8)()
    assert lib.ntt_modulus(cv.cid, out) == 0 and value(out) == cv.q
    assert lib.ntt_modulus(99, out) == -1


def test_plan_invariants(lib):
    assert lib.ntt_max_log2n() == 29
    assert 1 <= lib.ntt_default_tile_log() <= lib.ntt_max_tile_log()
    st = (C.c_int32 * 29)()
    for log2n in range(0, 30):
        for tile_log in range(1, lib.ntt_max_tile_log() + 1):
            p = lib.ntt_plan(log2n, tile_log, st)
            stages = list(st[:p])
            assert p == -(-log2n // tile_log), (log2n, tile_log)
            assert sum(stages) == log2n and all(1 <= t <= tile_log for t in stages), (log2n, tile_log, stages)


@pytest.mark.parametrize("name", D.NAMES)
def test_butterfly_at_the_ends_of_the_bounds(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    edge = (0, 1, q - 1, q, q + 1, TOP)
    ws = (0, 1, q - 1, O.prng_ints(f"ntt/host/w/{name}", 1, q)[0])
    ou, ov = (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
    for u, v in itertools.product(edge, edge):
        for w in ws:
            assert lib.ntt_butterfly(cv.cid, words(u), words(v), words(w), 1, ou, ov) == 0
            ru, rv = value(ou), value(ov)
            assert ru < 2 * q and rv < 2 * q, (name, u, v, w)
            assert ru % q == (u + w * v) % q and rv % q == (u - w * v) % q, (name, u, v, w)
        assert lib.ntt_butterfly(cv.cid, words(u), words(v), words(1), 0, ou, ov) == 0      # stage 0: no multiplication
        ru, rv = value(ou), value(ov)
        assert ru < 2 * q and rv < 2 * q
        assert ru % q == (u + v) % q and rv % q == (u - v) % q, (name, u, v)


def inputs(name, tag, n, q):
    vals = O.prng_ints(f"ntt/host/{name}/{tag}", n, 1 << 256)
    for i, s in zip(range(1, n, 3), itertools.cycle((q, q + 1, TOP, 0))):
        if i % 5 == 1:
            vals[i] = s
    return vals


@pytest.mark.parametrize("tile_log", [1, 2, 3, 10])
@pytest.mark.parametrize("name", ["bls377", "bn254"])
def test_executor_is_the_model(lib, name, tile_log):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    shift = O.prng_ints(f"ntt/host/{name}/shift", 1, q - 1)[0] + 1
    for log2n in range(0, 11):
        n = 1 << log2n
        a = inputs(name, f"exec/{log2n}", n, q)
        root = M.root_of_unity(q, log2n)
        # the library's root, forward and inverse, plain and coset; the second root on the coset forward
        for omega, sh, inv in ((root, None, False), (root, None, True), (root, shift, False), (root, shift, True),
                               (pow(root, 3, q), shift, False)):
            got = run(lib, cv, log2n, 1, tile_log, a, omega, sh, inv)
            assert got == M.ntt(a, q, omega, sh or 1, inv), (name, tile_log, log2n, sh is not None, inv)


@pytest.mark.parametrize("name", D.NAMES)
def test_executor_batches_on_every_field(lib, name):
    """B = 3 vectors back to back at the sizes every field has (log2n <= 1), and up to 2^7 with a 3-stage tile where q allows"""
    cv = D.CURVE_TABLE[name]
    q = cv.q
    for log2n in range(0, min(7, M.max_log2n(q)) + 1):
        n = 1 << log2n
        a = inputs(name, f"batch/{log2n}", 3 * n, q)
        for inv in (False, True):
            got = run(lib, cv, log2n, 3, 3, a, M.root_of_unity(q, log2n), None, inv)
            exp = [v for b in range(3) for v in M.ntt(a[b * n:(b + 1) * n], q, None, 1, inv)]
            assert got == exp, (name, log2n, inv)
