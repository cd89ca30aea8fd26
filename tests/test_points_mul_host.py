"""msm_points_mul / msm_points_mul_base on the CPU: the recoding and the lane bodies of montgomery_amd/csrc/points_mul.h compiled
for the host (tests/csrc/points_mul_host.hip), on all seven curves.

(i)   the recoding at every candidate window (3, 4, 5 of the variable base; 6, 8, 10 of the fixed base): the digits are those of
      window_step's carry rule restated here, sum d_j 2^(w j) is the half's magnitude, |d_j| <= 2^(w-1), nothing is left above
      the last window, and the signed halves recombine to the scalar mod q;
(ii)  the variable-base lane body bit for bit against the row of cv.scale(s, P), over table slots that are reused;
(iii) the fixed-base lane body over a table built through the variable-base body.
"""
import ctypes as C
import functools
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402
import digit_model as M  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

from host_lib import host_library, words  # noqa: E402

VAR_WIDTHS, BASE_WIDTHS = (3, 4, 5), (6, 8, 10)
TWO256 = 1 << 256


@pytest.fixture(scope="module")
def lib():
    L = host_library("points_mul_host")
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    L.pm_table_elems.argtypes = [C.c_int, C.c_int, C.c_uint64]
    L.pm_table_elems.restype = C.c_uint64
    L.pm_recode.argtypes = [C.c_int, C.c_int, u32p, u32p, i32p, i32p]
    L.pm_make_row.argtypes = [C.c_int, u32p, u32p]
    L.pm_lane.argtypes = [C.c_int, C.c_int, u32p, u32p, C.c_void_p, C.c_uint64, C.c_uint64, u32p]
    L.pm_base_table.argtypes = [C.c_int, C.c_int, u32p, u32p]
    L.pm_base_lane.argtypes = [C.c_int, C.c_int, u32p, u32p, u32p]
    return L


def value(ws):   # not host_lib.value: the whole array is one number, whatever its length
    return sum(int(w) << (32 * j) for j, w in enumerate(ws))


def edge_scalars(cv):
    """0, 1, 2, q - 2, q - 1, q, q + 1, 2^256 - 1; lambda and q - lambda (one half zero); the `low` / `high` lists of
    tests/digit_model.py."""
    q = cv.q
    out = [0, 1, 2, q - 2, q - 1, q, q + 1, TWO256 - 1]
    if not cv.te:
        out += [cv.B.lam, q - cv.B.lam]
    low, high = M.fixed_scalars(cv)
    return list(dict.fromkeys(out + low + high))


def pattern_scalars(cv, w, bits):
    """Scalars whose halves (the Edwards curve: the scalar) are all-ones, 0x88...8 and 0x77...7 below 2^(bits - 1): every window
    at or next to +-2^(w-1), carries rippling to the top; and the edge patterns of tests/digit_model.py at this window."""
    q = cv.q
    ones = (1 << (bits - 1)) - 1
    pats = [ones, int("8" * 64, 16) & ones, int("7" * 64, 16) & ones, ones >> 1, ones ^ (ones >> 3)]
    pats += M.patterns(w, -(-(bits + 1) // w), False, bits - 1)[:40]
    if cv.te:
        return [p % q for p in pats]
    lam = cv.B.lam
    out = []
    for i, h0 in enumerate(pats):
        h1 = pats[(3 * i + 1) % len(pats)]
        out += [(h0 + h1 * lam) % q, (h0 - h1 * lam) % q, (-h0 + h1 * lam) % q, (h1 * lam) % q, h0 % q]
    return out


def window_step_digits(mag, w, nwin):
    """The signed windows of `mag` by the carry rule of window_step (msm_kernels.h), least significant first, and the top carry."""
    L, carry, out = 1 << (w - 1), 0, []
    for k in range(nwin):
        l = ((mag >> (w * k)) & ((1 << w) - 1)) + carry
        if l > L:
            out.append(l - 2 * L)
            carry = 1
        else:
            out.append(l)
            carry = 0
    return out, carry + (mag >> (w * nwin))


def check_recoding(lib, cv, w, s):
    mw = lib.pm_max_win()
    mags, dig, info = (C.c_uint32 * 8)(), (C.c_int32 * (2 * mw))(), (C.c_int32 * 5)()
    assert lib.pm_recode(cv.cid, w, words(s, 8), mags, dig, info) == 0
    nwin, neg0, neg1, top0, top1 = info
    bits = lib.pm_chain_bits(cv.cid)
    assert nwin == -(-(bits + 1) // w) and nwin <= mw
    assert top0 == 0 and top1 == 0, "a carry left the last window"
    halves = [value(mags[:8])] if cv.te else [value(mags[:4]), value(mags[4:])]
    total = 0
    for e, mag in enumerate(halves):
        d = list(dig[e * mw:e * mw + nwin])
        assert mag < 1 << bits
        want, top = window_step_digits(mag, w, nwin)
        assert top == 0 and d == want, (cv.name, w, hex(s), e)
        assert sum(v << (w * j) for j, v in enumerate(d)) == mag
        assert max(abs(v) for v in d) <= 1 << (w - 1)
        total += (-mag if (neg0, neg1)[e] else mag) * (1 if e == 0 else cv.B.lam)
    assert (total - s) % cv.q == 0
    if cv.te:
        assert halves[0] == s % cv.q
    return halves


@pytest.mark.parametrize("name", D.NAMES)
def test_recoding_at_every_candidate_window(lib, name):
    cv = D.CURVE_TABLE[name]
    bits = lib.pm_chain_bits(cv.cid)
    assert bits == cv.scalar_bits
    rnd = O.prng_ints(f"points_mul/recode/{name}", 1000, cv.q)
    for w in VAR_WIDTHS + BASE_WIDTHS:
        for s in rnd + edge_scalars(cv) + pattern_scalars(cv, w, bits):
            check_recoding(lib, cv, w, s)


@pytest.mark.parametrize("name", [n for n in D.NAMES if n != "ed377"])
def test_lambda_leaves_one_half_zero(lib, name):
    cv = D.CURVE_TABLE[name]
    for w in VAR_WIDTHS:
        assert check_recoding(lib, cv, w, cv.B.lam) == [0, 1]
        assert check_recoding(lib, cv, w, cv.q - cv.B.lam) == [0, 1]
        assert check_recoding(lib, cv, w, 1) == [1, 0]


# ---------------------------------------------------------------------------------------------- the lane bodies

def make_row(lib, cv, P):
    """The resident row of an affine point (None / (0, 1): the identity), through the library's own base_row."""
    nw, rw = lib.pm_coord_words(cv.cid), lib.pm_row_words(cv.cid)
    row = (C.c_uint32 * rw)()
    if P is None:
        xy = words(0, 2 * nw)
    else:
        xy = words(P[0] | (P[1] << (32 * nw)), 2 * nw)
    assert lib.pm_make_row(cv.cid, xy, row) == 0
    return row


@functools.lru_cache(maxsize=None)
def _lincomb_row_maker():
    L = host_library("lincomb_host")
    u32p = C.POINTER(C.c_uint32)
    L.lc_make_row.argtypes = [C.c_int, u32p, u32p, C.c_int, u32p]
    return L


def wire_row(cv, P):
    """The row msm_set_points writes for P, from the shim that restates k_points_from_wire (tests/csrc/lincomb_host.hip)."""
    L = _lincomb_row_maker()
    nw = L.lc_coord_words(cv.cid)
    row = (C.c_uint32 * L.lc_row_words(cv.cid))()
    ident = P is None
    x, y = (0, 0) if ident else P
    assert L.lc_make_row(cv.cid, words(x, nw), words(y, nw), int(ident), row) == 0
    return list(row)


def new_table(lib, cv, w, cap):
    n = lib.pm_table_elems(cv.cid, w, cap) * 4
    return (C.c_uint32 * n)(*([0xA5A5A5A5] * n))


def lane(lib, cv, w, P, s, tbl, cap=1, g=0):
    out = (C.c_uint32 * lib.pm_row_words(cv.cid))()
    assert lib.pm_lane(cv.cid, w, make_row(lib, cv, P), words(s, 8), tbl, cap, g, out) == 0
    return list(out)


def expected_row(cv, s, P):
    if P is None or P == cv.zero:
        return wire_row(cv, cv.zero)
    return wire_row(cv, cv.scale(s % cv.q, P))


def lane_scalars(cv, n_random):
    q = cv.q
    sc = [0, 1, 2, q - 2, q - 1, q, q + 1, TWO256 - 1]
    if not cv.te:
        sc += [cv.B.lam, q - cv.B.lam]
    return sc + O.prng_ints(f"points_mul/lane/{cv.name}", n_random, q)


def test_the_row_maker_agrees_with_the_wire_rows(lib):
    for name in D.NAMES:
        cv = D.CURVE_TABLE[name]
        for P in (D.pool(name)[0][0], cv.zero):
            assert list(make_row(lib, cv, P)) == wire_row(cv, P)
        G = (cv.B.gx, cv.B.gy)
        row = (C.c_uint32 * lib.pm_row_words(cv.cid))()
        assert lib.pm_make_row(cv.cid, None, row) == 0 and list(row) == wire_row(cv, G)


@pytest.mark.parametrize("name", D.NAMES)
def test_variable_base_lane_equals_the_oracle_bit_for_bit(lib, name):
    """Every lane of one width runs over the SAME table slots, lane 1 of 3, with another point each time: no stale entry survives
    (identity rows leave the slots of the point before them untouched and must not read them)."""
    cv = D.CURVE_TABLE[name]
    pts = D.pool(name)[0]
    w = lib.pm_built_w()
    tbl = new_table(lib, cv, w, 3)
    i = 0
    for s in lane_scalars(cv, 6):
        for P in (pts[i % D.POOL], cv.zero) if i % 4 == 0 else (pts[i % D.POOL],):
            assert lane(lib, cv, w, P, s, tbl, 3, 1) == expected_row(cv, s, P), (name, hex(s), P is cv.zero)
        i += 1
    # the neighbours' slots were never written
    n = len(tbl)
    assert all(tbl[j] == 0xA5A5A5A5 for j in range(0, n, 12)) and all(tbl[j] == 0xA5A5A5A5 for j in range(8, n, 12))
    assert any(tbl[j] != 0xA5A5A5A5 for j in range(4, n, 12))


@pytest.mark.parametrize("name", ("bls377", "ed377"))
@pytest.mark.parametrize("w", VAR_WIDTHS)
def test_variable_base_lane_at_the_other_candidate_windows(lib, name, w):
    cv = D.CURVE_TABLE[name]
    pts = D.pool(name)[0]
    tbl = new_table(lib, cv, w, 1)
    for i, s in enumerate([1, cv.q - 1, TWO256 - 1] + O.prng_ints(f"points_mul/lane_w/{name}/{w}", 2, cv.q)):
        assert lane(lib, cv, w, pts[i], s, tbl) == expected_row(cv, s, pts[i])


@functools.lru_cache(maxsize=None)
def base_table(lib, name, w, which):
    cv = D.CURVE_TABLE[name]
    base = {"G": (cv.B.gx, cv.B.gy), "pool": D.pool(name)[0][7], "identity": cv.zero}[which]
    rows = lib.pm_base_table_rows(cv.cid, w)
    table = (C.c_uint32 * (rows * lib.pm_row_words(cv.cid)))()
    assert lib.pm_base_table(cv.cid, w, make_row(lib, cv, base), table) == 0
    return base, table


def check_base_lanes(lib, cv, w, which, scalars):
    base, table = base_table(lib, cv.name, w, which)
    for s in scalars:
        out = (C.c_uint32 * lib.pm_row_words(cv.cid))()
        assert lib.pm_base_lane(cv.cid, w, words(s, 8), table, out) == 0
        assert list(out) == expected_row(cv, s, base), (cv.name, w, which, hex(s))


@pytest.mark.parametrize("name", D.NAMES)
def test_fixed_base_lane_equals_the_oracle_bit_for_bit(lib, name):
    cv = D.CURVE_TABLE[name]
    w = lib.pm_built_wb()
    rw = lib.pm_row_words(cv.cid)
    base, table = base_table(lib, name, w, "pool")
    # the table itself: row (k, j - 1) = j 2^(w k) P
    L = 1 << (w - 1)
    top = lib.pm_base_table_rows(cv.cid, w) // L - 1
    j_top = min(L, (1 << (cv.scalar_bits + 1 - w * top)))      # the largest digit the top window can hold
    for k, j in ((0, 1), (0, L), (1, 1), (3, 5), (top, 1), (top, j_top)):
        at = (k * L + j - 1) * rw
        assert list(table[at:at + rw]) == expected_row(cv, j << (w * k), base), (name, k, j)
    check_base_lanes(lib, cv, w, "pool", lane_scalars(cv, 6))
    check_base_lanes(lib, cv, w, "G", lane_scalars(cv, 2))
    check_base_lanes(lib, cv, w, "identity", [0, 1, cv.q - 1, 12345])


@pytest.mark.parametrize("name", ("bls377", "ed377"))
def test_fixed_base_lane_at_the_other_candidate_windows(lib, name):
    cv = D.CURVE_TABLE[name]
    for w in (6, 10):
        check_base_lanes(lib, cv, w, "pool", [1, cv.q - 1, TWO256 - 1] + O.prng_ints(f"points_mul/base_w/{name}/{w}", 3, cv.q))
