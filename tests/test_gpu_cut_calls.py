"""Narrow, indexed, batched and wide MSMs through a CUT call: msm_set_workspace_limit makes group_schedule (msm_plan.hip) cut a
call into several window groups (a later group starts at k_lo != 0) or, tighter, every window into three ranges of the entries whose
sums window_sums_once adds on the host; run_fused sizes the groups of a batch from the same limit.  `-m gpu`.  (The schedules
themselves, without a GPU: tests/test_group_schedule.py.)

Every case has three assertions.  (1) The result is (sum_i value_i a_i mod q) G from the discrete logs a_i msm_generate_points
returns -- the check: a cut and an uncut call share their kernels.  (2) It equals the uncut call of the same entry point bit for
bit.  (3) The cut took place: the window-groups call reports more tree `rounds` than the uncut call and the ranges call more than
the window-groups call (at least 2 K single-window groups against at most K).  After every cut call the same context, without a
limit, returns the same element and the uncut `rounds` again.

The limits.  window_bytes (msm_plan.hip) of a window of the one-level sort over n entries is n * 233 bytes on the Weierstrass
curves (n * 113 on the Edwards curve) plus 2^(c-1) * (160 + 8 * CUs) for its buckets: at c = 10 and 256 CUs 1.13 MB.  A workspace
gets room = limit / 2.  Three ranges: room half way between window_bytes(n / 3) and window_bytes(n / 2) -- BLS12-377 at
n = 2^16 + 37: 21 858 * 233 + 1.13 MB = 6.22 MB and 32 787 * 233 + 1.13 MB = 8.77 MB, so room = 7.5 MB, limit = 15.0 MB; the
Edwards curve 3.60 MB and 4.84 MB, limit = 8.4 MB.  point_pieces then stops at three pieces and the ranges start at n / 3 = 21 857
and 2 n / 3 = 43 715, both odd: inside the dword a lane of the 1- and 2-byte formats loads.  Window groups only: room = 2.5
windows (1.5 where the call has two windows), so window_bytes(n) < room < K window_bytes(n) and the groups start at k_lo = 2, 4,
... (k_lo = 1).  The band of the ranges limit is +-16 % wide and a CU count other than 256 moves its ends by 2 % per 100 CUs; no
limit is trusted for that reason, every call proves its cut by (3).

The window is c = 10 (512 buckets: the per-bucket terms stay small next to n * 233) except for the 1-byte formats: 9 and 8 bits
under c = 10 are one window, which no limit cuts into groups, so they run c = 4 (unsigned, K = 3) and c = 7 (signed, K = 2).
A signed format declares a `bits` that c divides: the top window then holds the carry of the recoding and nothing else.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from operator_fixture import OperatorFixture  # noqa: E402

pytestmark = pytest.mark.gpu

N = (1 << 16) + 37     # resident points: n / 3 > 4096 (point_pieces cuts no further), n / 3 and 2 n / 3 odd
M3 = 3 * N + 5         # entries of an indexed call that names every point about three times
C10 = 10
B = 7
CURVES = ("bls377", "ed377")
# width -> (signed, bits, c), K = ceil((bits + 1) / c) >= 2 everywhere
NARROW = {1: ((False, 8, 4), (True, 7, 7)), 2: ((False, 16, 10), (True, 10, 10)), 4: ((False, 32, 10), (True, 30, 10)),
          8: ((False, 64, 10), (True, 60, 10)), 16: ((False, 128, 10), (True, 120, 10)), 32: ((False, 128, 10), (True, 120, 10))}


# ---------------------------------------------------------------------------------------------- points, shared by all tests

class Fix(OperatorFixture):
    def __init__(self, name):
        super().__init__(name)
        self.te = self.cv.te
        self.logs = self.ctx.generate_points(N, seed=1501, want_scalars=True)        # a_i of P_i = a_i G, N x 32 bytes
        self.logs_np = np.frombuffer(self.logs, dtype=np.uint8).reshape(N, 32)

    def log(self, i):
        return int.from_bytes(self.logs[32 * int(i):32 * int(i) + 32], "little")


_FIXES = {}


def _fix(name):
    if name not in _FIXES:
        _FIXES[name] = Fix(name)
    return _FIXES[name]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for f in _FIXES.values():
        f.ctx.close()
    _FIXES.clear()


# ---------------------------------------------------------------------------------------------- the limits

def _window_bytes(te, entries, c, n_cu=256):
    """window_bytes of msm_plan.hip for a window of the one-level sort (c <= 16)"""
    L = 1 << (c - 1)
    return entries * (113 if te else 233) + L * 160 + L * 8 * n_cu


def _limits(te, m, c, K):
    """msm_set_workspace_limit values (room = limit / 2, see the module docstring) for a call over m entries"""
    assert K >= 2 and m // 3 > 4096
    wpg = 2 if K >= 3 else 1
    return {"groups": int((2 * wpg + 1) * _window_bytes(te, m, c)),
            "ranges": _window_bytes(te, -(-m // 3), c) + _window_bytes(te, -(-m // 2), c)}


def _cut_starts(m):
    return [m // 3, 2 * m // 3]     # n q / pieces of group_schedule, pieces = 3


# ---------------------------------------------------------------------------------------------- references

def _k_signed(logs, vals, q):
    """sum_i vals_i a_i mod q for Python integers of either sign (a positive and a negative part through the C oracle)"""
    from oracle import c_oracle

    m = len(vals)
    k = c_oracle.dot_mod(logs, b"".join((v if v > 0 else 0).to_bytes(32, "little") for v in vals), m, q)
    if any(v < 0 for v in vals):
        k -= c_oracle.dot_mod(logs, b"".join((-v if v < 0 else 0).to_bytes(32, "little") for v in vals), m, q)
    return k % q


def _k_wide(logs, sc, q):
    """the same for an (m, 32) uint8 array of scalars"""
    from oracle import c_oracle

    return c_oracle.dot_mod(logs, sc.tobytes(), sc.shape[0], q)


def _assert_cut_is_live(k, val_at, log_at, starts, q):
    """The reference value of every WRONG cut near a range start differs from k.  A cut whose lower range ends at b + e and whose
    upper range starts at b + s counts entry j [j < b + e] + [j >= b + s] times; e = s is the same sum cut elsewhere, every
    other pair within three entries (a lane's dword holds up to four scalars) counts some entries twice or not at all."""
    for b in starts:
        t = {j: val_at(j) * log_at(j) % q for j in range(b - 3, b + 3)}
        for e in range(-3, 4):
            for s in range(-3, 4):
                k_cut = (k + sum(((j < b + e) + (j >= b + s) - 1) * tj for j, tj in t.items())) % q
                assert (k_cut == k) == (e == s), (b, e, s)


def _wide_scalars(rng, m):
    """m random scalars below 2^250 (< q on every curve here), none zero, as an (m, 32) uint8 array"""
    sc = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
    sc[:, 31] &= 3
    sc[:, 0] |= 1
    return sc


def _narrow_values(seed, m, bits, signed, starts):
    """m non-zero integers over the whole declared range; the three entries on either side of every range start hold the extremes
    of the format: 2^bits - 1, -2^bits (unsigned: the top bit alone) and 1."""
    from montgomery_amd import narrow as N_

    lo, hi = N_.value_range(bits, signed)
    w = np.random.default_rng(seed).integers(0, 1 << 62, size=(m, 3), dtype=np.int64).tolist()
    vals = [(lo + (a | b << 62 | c << 124) % (hi - lo)) or 1 for a, b, c in w]
    edge = [hi - 1, lo if signed else hi >> 1, 1]
    for b in starts:
        vals[b - 3:b] = edge
        vals[b:b + 3] = edge
    return vals


# ---------------------------------------------------------------------------------------------- one call, uncut and cut

def _run_cuts(f, label, m, c, K, call, k, limits=None):
    """call() -> (result, info) uncut, then under each limit, and uncut again after each; returns the uncut result"""
    expect = f.cv.scale_g(k)
    ref, info0 = call()
    assert f.point(ref) == expect, (label, "uncut", info0)
    assert (info0["c"], info0["K"]) == (c, K), (label, info0)
    limits = _limits(f.te, m, c, K) if limits is None else limits
    rounds = info0["rounds"]
    print(f"cut-call {f.name} {label}: uncut rounds={rounds}", end="")
    try:
        for cut, limit in limits.items():
            f.ctx.set_workspace_limit(limit)
            got, info = call()
            print(f"; {cut} limit={limit} rounds={info['rounds']}", end="")
            assert f.point(got) == expect, (label, cut, limit, info)
            assert got == ref, (label, cut, limit)
            assert info["rounds"] > rounds, (label, cut, limit, rounds, info["rounds"])     # the cut took place
            rounds = info["rounds"]
            f.ctx.set_workspace_limit(0)
            again, info2 = call()
            assert again == ref and info2["rounds"] == info0["rounds"], (label, cut, info0["rounds"], info2["rounds"])
    finally:
        f.ctx.set_workspace_limit(0)
        print()
    return ref


# ---------------------------------------------------------------------------------------------- 1: msm_run_narrow

@pytest.mark.parametrize("width", sorted(NARROW))
@pytest.mark.parametrize("name", CURVES)
def test_run_narrow_cut_into_groups_and_ranges(name, width):
    """Host arrays (first = 0: the ranges start at the odd entries 21 857 and 43 715) and device arrays -- those of the 1- and
    2-byte formats one element into their buffer, so that nar.first = 1 before group_scalars adds the range start."""
    from montgomery_amd import narrow as N_

    f = _fix(name)
    starts = _cut_starts(N)
    for signed, bits, c in NARROW[width]:
        vals = _narrow_values(1510 + width, N, bits, signed, starts)
        k = _k_signed(f.logs, vals, f.q)
        _assert_cut_is_live(k, lambda j: vals[j], f.log, starts, f.q)
        raw = N_.pack(vals, width, signed, f.q)
        K = -(-(bits + 1) // c)
        assert f.ctx.plan_narrow(N, bits, c=c) == (c, K)
        host = _run_cuts(f, f"narrow w={width} signed={signed} host", N, c, K,
                         lambda: f.ctx.run_narrow(raw, bits=bits, signed=signed, width=width, c=c), k)
        off = width if width <= 2 else 0
        p = f.ctx.device_alloc(len(raw) + 32)
        try:
            f.ctx.device_upload(p, b"\xff" * off + raw + b"\xff" * 16)
            dev = _run_cuts(f, f"narrow w={width} signed={signed} device+{off}", N, c, K,
                            lambda: f.ctx.run_narrow_device(p + off, N, width, bits, signed, c=c), k)
        finally:
            f.ctx.device_free(p)
        assert dev == host


# ---------------------------------------------------------------------------------------------- 2: msm_run_indexed

@pytest.mark.parametrize("m", [N, M3])
@pytest.mark.parametrize("name", CURVES + ("pallas",))
def test_indexed_cut_into_groups_and_ranges(name, m):
    """idx + p_lo and the payloads of a group, which name positions inside it: random indices with repeats, the same entries
    sorted by index (identical bytes), and a second range that names one point under one scalar -- a bucket of m / 3 entries per
    window that only that range sees.  Host and device input."""
    f = _fix(name)
    rng = np.random.default_rng(1520 + m % 97)
    starts = _cut_starts(m)
    idx = rng.integers(0, N, size=m, dtype=np.uint32)
    sc = _wide_scalars(rng, m)
    assert np.unique(idx).size < m
    order = np.argsort(idx, kind="stable")
    h_idx, h_sc = idx.copy(), sc.copy()
    h_idx[starts[0]:starts[1]] = idx[starts[0]]
    h_sc[starts[0]:starts[1]] = sc[starts[0]]
    c, K = f.ctx.plan(m, c=C10, no_tables=True)
    assert c == C10 and K >= 3
    results = {}
    for label, ii, ss in (("random", idx, sc), ("sorted", idx[order], sc[order]), ("heavy", h_idx, h_sc)):
        ii, ss = np.ascontiguousarray(ii), np.ascontiguousarray(ss)
        k = _k_wide(f.logs_np[ii].tobytes(), ss, f.q)
        _assert_cut_is_live(k, lambda j: int.from_bytes(ss[j].tobytes(), "little"), lambda j: f.log(ii[j]), starts, f.q)
        raw = ss.tobytes()
        results[label] = _run_cuts(f, f"indexed m={m} {label} host", m, c, K, lambda: f.ctx.msm_indexed(raw, ii, c=C10), k)
        d_s, d_i = f.ctx.device_alloc(32 * m), f.ctx.device_alloc(4 * m + 16)
        try:
            f.ctx.device_upload(d_s, raw)
            f.ctx.device_upload(d_i, bytes(4) + ii.tobytes())       # (4 bytes into the buffer: not 16-byte aligned)
            dev = _run_cuts(f, f"indexed m={m} {label} device", m, c, K, lambda: f.ctx.msm_indexed_device(d_s, d_i + 4, m, c=C10), k)
        finally:
            f.ctx.device_free(d_s)
            f.ctx.device_free(d_i)
        assert dev == results[label]
    assert results["sorted"] == results["random"]
    _, info = f.ctx.msm_indexed(h_sc.tobytes(), h_idx, c=C10)
    assert info["max_bucket"] >= starts[1] - starts[0], info       # the heavy bucket is there


# ---------------------------------------------------------------------------------------------- 3: msm_run_indexed_narrow

@pytest.mark.parametrize("width", [1, 8])
@pytest.mark.parametrize("name", CURVES)
def test_indexed_narrow_cut_into_groups_and_ranges(name, width):
    """Both offsets at once: nar.first + p_lo for the scalars, idx + p_lo for the indices (signed values; the device form of the
    1-byte format starts one element into its buffer)."""
    from montgomery_amd import narrow as N_

    f = _fix(name)
    signed, bits, c = NARROW[width][1]
    K = -(-(bits + 1) // c)
    for m in (N, M3):
        starts = _cut_starts(m)
        idx = np.random.default_rng(1530 + width + m % 97).integers(0, N, size=m, dtype=np.uint32)
        vals = _narrow_values(1531 + width, m, bits, signed, starts)
        k = _k_signed(f.logs_np[idx].tobytes(), vals, f.q)
        _assert_cut_is_live(k, lambda j: vals[j], lambda j: f.log(idx[j]), starts, f.q)
        raw = N_.pack(vals, width, signed, f.q)
        assert f.ctx.plan_narrow(m, bits, c=c) == (c, K)
        host = _run_cuts(f, f"indexed-narrow w={width} m={m} host", m, c, K,
                         lambda: f.ctx.msm_indexed_narrow(raw, idx, bits=bits, signed=signed, width=width, c=c), k)
        off = 1 if width == 1 else 0
        d_s, d_i = f.ctx.device_alloc(len(raw) + 32), f.ctx.device_alloc(4 * m + 16)
        try:
            f.ctx.device_upload(d_s, b"\xff" * off + raw + b"\xff" * 16)
            f.ctx.device_upload(d_i, bytes(4) + idx.tobytes())
            dev = _run_cuts(f, f"indexed-narrow w={width} m={m} device+{off}", m, c, K,
                            lambda: f.ctx.msm_indexed_narrow_device(d_s + off, d_i + 4, m, width, bits=bits, signed=signed, c=c), k)
        finally:
            f.ctx.device_free(d_s)
            f.ctx.device_free(d_i)
        assert dev == host


# ---------------------------------------------------------------------------------------------- 4: fused batches

def _batch_limits(te, c, K):
    """run_fused: wpg = limit / 2 / window_bytes(n) windows, per = wpg / K elements.  2.5 K windows: two elements per group, four
    groups for B = 7; K / 2 windows: below one element, per = 1, seven groups."""
    return {"two": 5 * K * _window_bytes(te, N, c), "one": K * _window_bytes(te, N, c)}


def _run_batch_cuts(f, label, c, K, call, single, ks):
    """call() -> [(result, info)] * B; every element against its own discrete-log value and against `single(b)`, the element
    alone without a limit; more groups, more rounds"""
    expect = [f.cv.scale_g(k) for k in ks]
    alone = [single(b) for b in range(B)]
    got0 = call()
    assert [f.point(r) for r, _ in got0] == expect, (label, "no limit")
    assert [r for r, _ in got0] == alone
    assert (got0[0][1]["c"], got0[0][1]["K"]) == (c, K)
    rounds = got0[0][1]["rounds"]
    print(f"cut-call {f.name} {label}: no limit rounds={rounds}", end="")
    try:
        for cut, limit in _batch_limits(f.te, c, K).items():
            f.ctx.set_workspace_limit(limit)
            got = call()
            print(f"; {cut} limit={limit} rounds={got[0][1]['rounds']}", end="")
            assert [f.point(r) for r, _ in got] == expect, (label, cut, limit)
            assert [r for r, _ in got] == alone, (label, cut, limit)
            assert got[0][1]["rounds"] > rounds, (label, cut, limit, rounds, got[0][1]["rounds"])
            rounds = got[0][1]["rounds"]
            f.ctx.set_workspace_limit(0)
            again = call()
            assert [r for r, _ in again] == alone and again[0][1]["rounds"] == got0[0][1]["rounds"], (label, cut)
    finally:
        f.ctx.set_workspace_limit(0)
        print()


@pytest.mark.parametrize("name", CURVES)
def test_batch_groups_sized_by_the_limit(name):
    f = _fix(name)
    rng = np.random.default_rng(1540)
    sc = [_wide_scalars(rng, N) for _ in range(B)]
    raws = [s.tobytes() for s in sc]
    c, K = f.ctx.plan(N, c=C10, no_tables=True)
    _run_batch_cuts(f, "batch", c, K, lambda: f.ctx.run_batch(raws, c=C10, no_tables=True),
                    lambda b: f.ctx.run(raws[b], c=C10, no_tables=True)[0], [_k_wide(f.logs, s, f.q) for s in sc])


@pytest.mark.parametrize("width", [1, 8])
@pytest.mark.parametrize("name", CURVES)
def test_batch_narrow_groups_sized_by_the_limit(name, width):
    from montgomery_amd import narrow as N_

    f = _fix(name)
    signed = width == 1
    _, bits, c = NARROW[width][1 if signed else 0]
    K = -(-(bits + 1) // c)
    vals = [_narrow_values(1550 + 10 * width + b, N, bits, signed, _cut_starts(N)) for b in range(B)]
    raws = [N_.pack(v, width, signed, f.q) for v in vals]
    kw = dict(bits=bits, signed=signed, width=width, c=c)
    _run_batch_cuts(f, f"batch-narrow w={width}", c, K, lambda: f.ctx.run_batch_narrow(raws, **kw),
                    lambda b: f.ctx.run_narrow(raws[b], **kw)[0], [_k_signed(f.logs, v, f.q) for v in vals])


# ---------------------------------------------------------------------------------------------- 5: refusals through a cut

@pytest.mark.parametrize("name", CURVES)
def test_refusals_through_a_cut(name):
    """The error word is raised by whichever range saw the bad value and read once, after all groups ran; an index >= n is
    refused before any range runs.  The same context, still under the limit, then returns the right element for clean input."""
    from montgomery_amd import _lib
    from montgomery_amd._lib import MsmOpts, MsmResult
    from montgomery_amd.api import MsmError

    f = _fix(name)
    starts = _cut_starts(N)
    try:
        # a narrow value outside the declared bits, in the last range only
        signed, bits, c = NARROW[4][1]
        K = -(-(bits + 1) // c)
        vals = _narrow_values(1560, N, bits, signed, starts)
        good = np.array(vals, dtype=np.int32)
        expect = f.cv.scale_g(_k_signed(f.logs, vals, f.q))
        uncut, info0 = f.ctx.run_narrow(good, bits=bits, c=c)
        f.ctx.set_workspace_limit(_limits(f.te, N, c, K)["ranges"])
        for at, v in ((N - 2, 1 << bits), (starts[1] + 1, -(1 << bits) - 1)):
            bad = good.copy()
            bad[at] = v
            with pytest.raises(MsmError) as e:
                f.ctx.run_narrow(bad, bits=bits, c=c)
            assert e.value.code == _lib.MSM_ERR_SCALAR, e.value
            got, info = f.ctx.run_narrow(good, bits=bits, c=c)
            assert f.point(got) == expect and got == uncut and info["rounds"] > info0["rounds"]
        f.ctx.set_workspace_limit(0)

        # a scalar >= q under msm_opts.strict, in the middle range of a wide call
        sc = _wide_scalars(np.random.default_rng(1561), N)
        c, K = f.ctx.plan(N, c=C10, no_tables=True)
        expect = f.cv.scale_g(_k_wide(f.logs, sc, f.q))
        uncut, info0 = f.ctx.run(sc.tobytes(), c=C10, no_tables=True)
        over = sc.copy()
        over[N // 2] = np.frombuffer((f.q + 5).to_bytes(32, "little"), dtype=np.uint8)
        assert starts[0] < N // 2 < starts[1]
        f.ctx.set_workspace_limit(_limits(f.te, N, c, K)["ranges"])
        res = MsmResult()
        for rows, want in ((over, _lib.MSM_ERR_SCALAR), (sc, _lib.MSM_OK)):
            buf = (ctypes.c_uint8 * (32 * N)).from_buffer_copy(rows.tobytes())
            rc = f.ctx._lib.msm_run(f.ctx._h, buf, N, 0, ctypes.byref(MsmOpts(c=C10, strict=1, no_tables=1)), ctypes.byref(res))
            assert rc == want, (rc, want)
        assert f.ctx._affine(res) == uncut and f.point(uncut) == expect and res.rounds > info0["rounds"]
        f.ctx.set_workspace_limit(0)

        # an index >= n in the last third of an indexed call
        m = M3
        idx = np.random.default_rng(1562).integers(0, N, size=m, dtype=np.uint32)
        sc = _wide_scalars(np.random.default_rng(1563), m)
        c, K = f.ctx.plan(m, c=C10, no_tables=True)
        expect = f.cv.scale_g(_k_wide(f.logs_np[idx].tobytes(), sc, f.q))
        uncut, info0 = f.ctx.msm_indexed(sc.tobytes(), idx, c=C10)
        f.ctx.set_workspace_limit(_limits(f.te, m, c, K)["ranges"])
        at = _cut_starts(m)[1] + 12345
        bad = idx.copy()
        bad[at] = N
        with pytest.raises(MsmError) as e:
            f.ctx.msm_indexed(sc.tobytes(), bad, c=C10)
        assert e.value.code == _lib.MSM_ERR_ARG and f"indices[{at}] = {N}" in str(e.value), str(e.value)
        got, info = f.ctx.msm_indexed(sc.tobytes(), idx, c=C10)
        assert f.point(got) == expect and got == uncut and info["rounds"] > info0["rounds"]
    finally:
        f.ctx.set_workspace_limit(0)


# ---------------------------------------------------------------------------------------------- 6: the wide dense call

@pytest.mark.parametrize("name", CURVES)
def test_wide_call_cut_into_window_groups(name):
    """msm_run on the plain path at c = 10 (BLS12-377: K = 13 after GLV): groups of two windows, k_lo = 2, 4, ... on the one-level
    sort -- and the three ranges at this window, next to the c = 12 / 13 of tests/test_gpu_boundary.py.  Host and device scalars."""
    f = _fix(name)
    sc = _wide_scalars(np.random.default_rng(1570), N)
    raw = sc.tobytes()
    k = _k_wide(f.logs, sc, f.q)
    _assert_cut_is_live(k, lambda j: int.from_bytes(sc[j].tobytes(), "little"), f.log, _cut_starts(N), f.q)
    c, K = f.ctx.plan(N, c=C10, no_tables=True)
    assert K == (26 if f.te else 13)
    host = _run_cuts(f, "wide host", N, c, K, lambda: f.ctx.run(raw, c=C10, no_tables=True), k)
    p = f.ctx.device_alloc(32 * N)
    try:
        f.ctx.device_upload(p, raw)
        dev = _run_cuts(f, "wide device", N, c, K, lambda: f.ctx.run_device(p, N, c=C10, no_tables=True), k)
    finally:
        f.ctx.device_free(p)
    assert dev == host
