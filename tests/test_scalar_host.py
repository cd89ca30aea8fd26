"""The host side of the scalar field (montgomery_amd/csrc/scalar_host.h) and the range and row rules of operator_checks.h on the
CPU (tests/csrc/scalar_host_host.hip), over the scalar field the dispatch gives each of the seven curves, against Python integers
mod cv.q: how a call's scalars are read and refused, the two-adicity, the non-residue, the library's roots of unity, the inverses
and the power tables the kernels take as arguments.  Registers hold Montgomery forms under R = 2^270."""
import ctypes as C
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

from host_lib import host_library, value, words  # noqa: E402

R = 1 << 270
MSM_OK, MSM_ERR_ARG, MSM_ERR_SCALAR = 0, 1, 6   # include/msm_hip.h


@pytest.fixture(scope="module")
def lib():
    L = host_library("scalar_host_host")
    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    L.sh_modulus.argtypes = [C.c_int, u32p]
    L.sh_parse.argtypes = [C.c_int, u8p, u32p, u32p, u32p, u8p]
    L.sh_two_adicity.argtypes = [C.c_int]
    L.sh_non_residue.argtypes = [C.c_int]
    L.sh_non_residue.restype = C.c_int64
    L.sh_library_root.argtypes = [C.c_int, C.c_uint32, u32p]
    L.sh_inverse.argtypes = [C.c_int, u32p, u32p]
    L.sh_inverse_n.argtypes = [C.c_int, C.c_uint32, u32p]
    L.sh_pow_table.argtypes = [C.c_int, u32p, C.c_int, u32p]
    L.sh_scalar_too_big.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    L.sh_dst_ranges_ok.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p, C.c_int]
    L.sh_rows_overlap_ok.argtypes = [C.c_uint64, C.c_uint64]
    return L


def two_adicity(q):
    return ((q - 1) & -(q - 1)).bit_length() - 1


def non_residue(q):
    return next(g for g in range(2, 64) if pow(g, (q - 1) // 2, q) == q - 1)


def random_scalar(cv, tag):
    return O.prng_ints(f"scalar_host/{tag}/{cv.name}", 1, cv.q)[0]


@pytest.mark.parametrize("name", D.NAMES)
def test_dispatched_field_is_the_group_order(lib, name):
    cv = D.CURVE_TABLE[name]
    out = (C.c_uint32 * 8)()
    assert lib.sh_modulus(cv.cid, out) == 0
    assert value(out) == cv.q
    assert lib.sh_modulus(99, out) == -2


@pytest.mark.parametrize("name", D.NAMES)
def test_parse_accepts_exactly_the_values_below_q(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    assert q & 0xFFFFFFFF, "the case below needs a lowest word of q that is not 0"
    # (q - 1 is also the value that equals q in the top seven words and is one below it in the lowest; one more case lies a whole
    # word below q, and one differs from q in the top word alone)
    cases = [0, 1, q - 1, q, q + 1, (1 << 256) - 1, q - (1 << 32), q - (1 << 224), q + (1 << 224), random_scalar(cv, "parse")]
    assert (q - 1) >> 32 == q >> 32 and (q - 1) & 0xFFFFFFFF == (q & 0xFFFFFFFF) - 1
    for v in cases:
        raw = v.to_bytes(32, "little")
        w, canon, mont = (C.c_uint32 * 8)(), (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
        back = (C.c_uint8 * 32)()
        rc = lib.sh_parse(cv.cid, (C.c_uint8 * 32)(*raw), w, canon, mont, back)
        assert rc == (1 if v < q else 0), hex(v)
        assert value(w) == v and bytes(back) == raw
        if v < q:
            assert value(canon) == v
            assert value(mont) == v * R % q


def test_the_refusal_of_a_scalar(lib):
    msg = C.create_string_buffer(256)
    assert lib.sh_scalar_too_big(b"msm_scalars_powers", b"x", msg, 256) == MSM_ERR_SCALAR
    assert msg.value == b"msm_scalars_powers: x >= q (scalars of this call are never reduced)"


@pytest.mark.parametrize("name", D.NAMES)
def test_two_adicity_and_non_residue(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    s = lib.sh_two_adicity(cv.cid)
    assert s == two_adicity(q) and (q - 1) % (1 << s) == 0 and ((q - 1) >> s) & 1
    g = lib.sh_non_residue(cv.cid)
    assert pow(g, (q - 1) // 2, q) == q - 1
    assert all(pow(h, (q - 1) // 2, q) != q - 1 for h in range(2, g))


@pytest.mark.parametrize("name", D.NAMES)
def test_library_root(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    g, s = non_residue(q), two_adicity(q)
    out = (C.c_uint32 * 8)()
    for log2n in sorted({0, 1, 2, 9, 10, 11, s}):
        assert lib.sh_library_root(cv.cid, log2n, out) == 0
        w = value(out)
        assert w == pow(g, (q - 1) >> log2n, q), log2n
        if log2n <= s:   # (the Edwards curve's order has two-adicity 1: beyond it the exponent is no divisor's, and nothing asks)
            assert pow(w, 1 << log2n, q) == 1 and (log2n == 0 or pow(w, 1 << (log2n - 1), q) == q - 1)


@pytest.mark.parametrize("name", D.NAMES)
def test_inverses(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    out = (C.c_uint32 * 8)()
    for a in (1, 2, q - 1, random_scalar(cv, "inverse")):
        assert lib.sh_inverse(cv.cid, words(a), out) == 0
        assert value(out) < q and value(out) * a % q == 1
    for k in (0, 1, 29):
        assert lib.sh_inverse_n(cv.cid, k, out) == 0
        assert value(out) < q and (value(out) << k) % q == 1


@pytest.mark.parametrize("name", D.NAMES)
def test_power_tables(lib, name):
    cv = D.CURVE_TABLE[name]
    q = cv.q
    for bits in (30, 40):   # sv::PowTable of k_sv_powers, scan::PowTab of the scans
        out = (C.c_uint32 * (8 * bits))()
        for x in (0, 1, q - 1, random_scalar(cv, "table")):
            assert lib.sh_pow_table(cv.cid, words(x), bits, out) == 0
            for k in range(bits):
                assert value(out, k) == pow(x, 1 << k, q) * R % q, (bits, k)
    assert lib.sh_pow_table(cv.cid, words(1), 31, out) == -1


def test_byte_ranges(lib):
    """dst may be the source itself or disjoint from it; an adjacent range is disjoint, a partial overlap is refused."""
    src = 1 << 20
    msg = C.create_string_buffer(256)

    def ok(dst, n):
        rc = lib.sh_dst_ranges_ok(dst, src, 32 * n, msg, 256)
        assert rc in (MSM_OK, MSM_ERR_ARG)
        if rc:
            assert msg.value == b"sh: dst overlaps a in part (it may be a itself or disjoint from it)"
        return rc == MSM_OK

    for n in (0, 1, 3):
        assert ok(src, n)
        assert ok(src + 32 * n, n) and ok(src - 32 * n, n)
        if n >= 2:
            for d in (16, 32 * (n - 1)):
                assert not ok(src + d, n) and not ok(src - d, n)
    assert not ok(src + 16, 1) and not ok(src - 16, 1)   # (half an element)
    assert ok(src + 16, 0)                               # (nothing is read or written)


def test_rows_of_a_source_inside_the_destination(lib):
    for count in (0, 1, 4):
        for lo in sorted({0, 1, max(count - 1, 0), count, count + 1}):
            assert lib.sh_rows_overlap_ok(lo, count) == (1 if count == 0 or lo == 0 or lo >= count else 0), (lo, count)
