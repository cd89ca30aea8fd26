"""msm_run_indexed / msm_run_indexed_narrow: sum_j s_j P[idx_j] over a chosen multiset of the resident points.  `-m gpu`.

Points come from msm_generate_points, which returns the discrete logs a_i of P_i = a_i G, so every case has the expected value
(sum_j s_j a_(idx_j) mod q) G from the oracle, and next to it compares bitwise with msm_run over the dense equivalent
(t[i] = sum of s_j over idx_j == i, mod q)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degenerate_inputs as D  # noqa: E402
from operator_fixture import OperatorFixture  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

N7 = 2048         # resident points of the all-curves fixture
N13 = 1 << 13     # of the BLS12-377 fixture that walks the sort paths


class Fix(OperatorFixture):
    def __init__(self, name, n, seed):
        super().__init__(name)
        self.n = n
        self.logs = O.scalars_from_bytes(self.ctx.generate_points(n, seed=seed, want_scalars=True))

    def dlog(self, idx, sc, logs=None):
        logs = self.logs if logs is None else logs
        return self.cv.scale_g(sum(int(s) * logs[int(i)] for i, s in zip(idx, sc)) % self.q)

    def check(self, idx, sc, logs=None, n=None, **kw):
        """indexed == the discrete-log value == msm_run over the dense equivalent, bit for bit; returns (result, info)"""
        from montgomery_amd import api

        n = self.n if n is None else n
        idx = np.asarray(idx, dtype=np.uint32)
        raw = O.scalars_to_bytes([int(s) for s in sc])
        got, info = self.ctx.msm_indexed(raw, idx, **kw)
        assert self.point(got) == self.dlog(idx, sc, logs), (self.name, len(sc), kw, info)
        dense, _ = self.ctx.run(api.dense_from_sparse(idx, raw, n, self.q), c=kw.get("c"), no_glv=kw.get("no_glv", False), no_tables=True)
        assert got == dense, (self.name, len(sc), kw, info)
        assert not info["tables"]
        return got, info


@pytest.fixture(scope="module", params=D.NAMES)
def f7(request):
    f = Fix(request.param, N7, seed=1301)
    yield f
    f.ctx.close()


@pytest.fixture(scope="module")
def f13():
    f = Fix("bls377", N13, seed=1302)
    yield f
    f.ctx.close()


def _ints(tag, n, bound):
    return O.prng_ints(f"indexed/{tag}", n, bound)


# ---------------------------------------------------------------------------------------------- 1: the smallest calls

def test_empty_single_and_doubled_entry(f7):
    f, q = f7, f7.q
    ident = f.ctx.run(bytes(32 * f.n), no_tables=True)[0]
    got, info = f.ctx.msm_indexed(b"", np.zeros(0, dtype=np.uint32))
    assert got == ident and f.point(got) == f.cv.zero
    assert (info["c"], info["K"]) == f.ctx.plan(0, no_tables=True)
    s = _ints(f"{f.name}/one", 3, q)
    f.check([0], [s[0]])
    f.check([f.n - 1], [s[1]])
    f.check([f.n - 1], [0])
    got, _ = f.check([7, 7], [s[2], s[2]])
    assert f.point(got) == f.cv.scale_g(2 * s[2] * f.logs[7])


# ---------------------------------------------------------------------------------------------- 2: more entries than points

def test_more_entries_than_resident_points(f7):
    f = f7
    f.ctx.pointset_create()
    try:
        logs = O.scalars_from_bytes(f.ctx.generate_points(300, seed=1303, want_scalars=True))
        idx = _ints(f"{f.name}/300", 1000, 300)
        assert len(set(idx)) < 300 or max(idx.count(i) for i in set(idx)) > 1
        _, info = f.check(idx, _ints(f"{f.name}/300s", 1000, f.q), logs=logs, n=300)
        assert (info["c"], info["K"]) == f.ctx.plan(1000, no_tables=True)   # the window of m = 1000, not of the 300 points
    finally:
        f.ctx.pointset_destroy(f.ctx._cur_set)


# ---------------------------------------------------------------------------------------------- 3: one point, many times

def test_all_indices_the_same_point(f7):
    f, q, m = f7, f7.q, 512
    sc = _ints(f"{f.name}/same", m, q)
    sc[-1] = (-sum(sc[:-1])) % q
    got, _ = f.check([5] * m, sc)
    assert f.point(got) == f.cv.zero                       # the scalars sum to 0 mod q
    sc[-1] = (12345 - sum(sc[:-1])) % q
    got, _ = f.check([5] * m, sc)
    assert f.point(got) == f.cv.scale_g(12345 * f.logs[5])
    got, _ = f.check([5] * m, [3] * m)                      # one bucket holds all of it: doublings all the way down
    assert f.point(got) == f.cv.scale_g(3 * m * f.logs[5])


# ---------------------------------------------------------------------------------------------- 4: cancelling pairs

def test_cancelling_pairs_among_random_entries(f7):
    f, q = f7, f7.q
    idx = _ints(f"{f.name}/ci", 600, f.n)
    sc = _ints(f"{f.name}/cs", 600, q)
    keep_idx, keep_sc = list(idx[:400]), list(sc[:400])
    all_idx, all_sc = list(keep_idx), list(keep_sc)
    for j, (i, s) in enumerate(zip(idx[400:500], sc[400:500])):   # (i, s) and (i, q - s) at scattered places
        s = s or 1
        all_idx.insert((37 * j) % len(all_idx), i); all_sc.insert((37 * j) % len(all_sc), s)
        all_idx.insert((91 * j + 5) % len(all_idx), i); all_sc.insert((91 * j + 5) % len(all_sc), q - s)
    got, _ = f.check(all_idx, all_sc)
    assert f.point(got) == f.dlog(keep_idx, keep_sc)
    only, _ = f.check([9, 9, 11, 11], [4, q - 4, q - 1, 1])
    assert f.point(only) == f.cv.zero


# ---------------------------------------------------------------------------------------------- 5: degenerate point sets

@pytest.mark.parametrize("name", ["bls377", "ed377", "pallas"])
def test_point_set_with_identities_and_negated_duplicates(name):
    """tests/degenerate_inputs.py: the identity at both ends and in a run, runs of one point and of Q, -Q alternating."""
    from montgomery_amd import api
    from montgomery_amd.api import MsmContext

    cv, lay = D.CURVE_TABLE[name], D.layout(1000)
    ctx = MsmContext(cv.cid)
    try:
        ctx.set_points(cv.wire(D.points_of(cv, lay.entries)))
        m = 1500
        idx = _ints(f"deg/{name}", m, lay.n)
        start, length, _kind = lay.runs[len(lay.runs) // 2 + 3]           # an alternating run, every entry of it twice
        idx[:2 * length] = [start + t // 2 for t in range(2 * length)]
        idx[-3:] = [0, lay.n - 1, lay.ident_run[0]]                       # identities
        sc = _ints(f"deg/{name}/s", m, cv.q)
        sc[:2 * length] = [sc[0]] * (2 * length)                          # one scalar over Q, Q, -Q, -Q, ...: all but the last pair cancel
        raw = O.scalars_to_bytes(sc)
        exp = D.expected(cv, [lay.entries[i] for i in idx], sc)
        for kw in ({}, {"c": 8}, {"c": 18}):
            got, info = ctx.msm_indexed(raw, idx, **kw)
            assert ((got.x, got.y) if cv.te else got.as_tuple()) == exp, (name, kw, info)
            dense, _ = ctx.run(api.dense_from_sparse(idx, raw, lay.n, cv.q), c=kw.get("c"), no_tables=True)
            assert got == dense, (name, kw)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 6: the sort paths, the tail rounds

@pytest.mark.parametrize("c", [8, 16, 18, 21])
def test_forced_windows_walk_every_sort_path(f13, c):
    """c <= 16: the one-level sort; 18 (folded top window) and 21: the bin split, k_bin_slots."""
    f, m = f13, 4096
    idx = _ints(f"paths/{c}/i", m, f.n)
    _, info = f.check(idx, _ints(f"paths/{c}/s", m, f.q), c=c)
    assert info["c"] == c and (info["c"], info["K"]) == f.ctx.plan(m, c=c, no_tables=True)


def test_without_the_endomorphism(f13):
    f, m = f13, 4096
    idx = _ints("paths/noglv/i", m, f.n)
    sc = _ints("paths/noglv/s", m, f.q)
    got, info = f.check(idx, sc, no_glv=True)
    assert info["K"] > f.ctx.plan(m, no_tables=True)[1]
    assert got == f.check(idx, sc)[0]


@pytest.mark.parametrize("c", [None, 16, 21])
def test_one_scalar_repeated_over_random_indices(f13, c):
    """Every entry of a window in one bucket: the heavy bin of the bin split (c = 21), the deepest tail rounds."""
    f, m = f13, 1 << 14
    one = _ints("heavy/s", 1, f.q)[0]
    idx = _ints("heavy/i", m, f.n)
    got, info = f.ctx.msm_indexed(O.scalars_to_bytes([one]) * m, np.asarray(idx, dtype=np.uint32), c=c)
    assert info["max_bucket"] >= m // 2, info
    assert f.point(got) == f.cv.scale_g(one * sum(f.logs[i] for i in idx))
    cnt = np.bincount(idx, minlength=f.n)
    dense = O.scalars_to_bytes([one * int(k) % f.q for k in cnt])
    assert got == f.ctx.run(dense, c=c, no_tables=True)[0]


def test_radix_split(f13):
    """2^20 entries over 2^13 points: 2^21 sort entries per window at c = 16 take the radix split; every point is named ~128
    times.  Scalars of 64 bits keep the host-side sums cheap; the GLV split still spreads them over both halves."""
    f, m = f13, 1 << 20
    rng = np.random.default_rng(1304)
    idx = rng.integers(0, f.n, size=m, dtype=np.uint32)
    s64 = rng.integers(0, (1 << 64) - 1, size=m, dtype=np.uint64, endpoint=True)
    raw = np.zeros((m, 32), dtype=np.uint8)
    raw[:, :8] = s64.view(np.uint8).reshape(m, 8)
    got, info = f.ctx.msm_indexed(raw, idx, c=16)
    per_point = [0] * f.n
    for i, s in zip(idx.tolist(), s64.tolist()):
        per_point[i] += s
    assert f.point(got) == f.cv.scale_g(sum(t * a for t, a in zip(per_point, f.logs)) % f.q), info
    assert got == f.ctx.run(O.scalars_to_bytes([t % f.q for t in per_point]), c=16, no_tables=True)[0]


# ---------------------------------------------------------------------------------------------- 7: the order does not matter

def test_sorted_and_permuted_entries_give_identical_bytes(f7):
    f, m = f7, 1024
    idx = sorted(_ints(f"{f.name}/perm/i", m, f.n))
    sc = _ints(f"{f.name}/perm/s", m, f.q)
    a, _ = f.check(idx, sc)
    perm = np.random.default_rng(7).permutation(m)
    b, _ = f.ctx.msm_indexed(O.scalars_to_bytes([sc[j] for j in perm]), np.asarray([idx[j] for j in perm], dtype=np.uint32))
    assert a == b


# ---------------------------------------------------------------------------------------------- 8: every curve

def test_every_curve_at_1024_of_2048(f7):
    f, m = f7, 1024
    idx = _ints(f"{f.name}/all/i", m, f.n)
    sc = _ints(f"{f.name}/all/s", m, f.q)
    _, info = f.check(idx, sc)
    assert (info["c"], info["K"]) == f.ctx.plan(m, no_tables=True)
    distinct = np.random.default_rng(8).permutation(f.n)[:m]          # the sparse-column shape: distinct positions
    f.check(distinct, sc)
    f.check(idx, sc, serial=True)


# ---------------------------------------------------------------------------------------------- 9: narrow scalars

def _narrow_dense(vals, idx, n):
    t = [0] * n
    for i, v in zip(idx, vals):
        t[int(i)] += int(v)
    return t


@pytest.mark.parametrize("name", ["bls377", "ed377"])
def test_narrow_forms(name):
    from montgomery_amd import narrow as N

    f = Fix(name, N7, seed=1305)
    try:
        m = 1000
        rng = np.random.default_rng(9)
        idx = rng.integers(0, f.n, size=m, dtype=np.uint32)
        # width 1 unsigned; the per-point sums need more than 8 bits, so the dense equivalent goes through msm_run
        u8 = rng.integers(0, 255, size=m, dtype=np.uint8, endpoint=True)
        u8[:2] = (255, 0)
        got, info = f.ctx.msm_indexed_narrow(u8, idx)
        assert f.point(got) == f.dlog(idx, u8.tolist()) and (info["c"], info["K"]) == f.ctx.plan_narrow(m, 8)
        assert got == f.ctx.run(N.widen(_narrow_dense(u8, idx, f.n), f.q), no_tables=True)[0]
        # width 8 unsigned, bits = 40, distinct positions: the dense equivalent is a narrow vector of the same format
        pos = rng.permutation(f.n)[:m].astype(np.uint32)
        u40 = rng.integers(0, (1 << 40) - 1, size=m, dtype=np.uint64, endpoint=True)
        u40[:2] = ((1 << 40) - 1, 0)
        got, info = f.ctx.msm_indexed_narrow(u40, pos, bits=40)
        assert f.point(got) == f.dlog(pos, u40.tolist()) and (info["c"], info["K"]) == f.ctx.plan_narrow(m, 40)
        dense = np.zeros(f.n, dtype=np.uint64)
        dense[pos] = u40
        assert got == f.ctx.run_narrow(dense, bits=40)[0]
        assert got == f.ctx.msm_indexed_narrow(u40, pos, bits=40, c=7)[0]
        # width 4 signed with negative values, repeats among the positions
        i32 = rng.integers(-(1 << 31), (1 << 31) - 1, size=m, dtype=np.int32, endpoint=True)
        i32[:3] = (-(1 << 31), (1 << 31) - 1, -1)
        got, _ = f.ctx.msm_indexed_narrow(i32, idx)
        assert f.point(got) == f.dlog(idx, i32.tolist())
        assert got == f.ctx.run(N.widen(_narrow_dense(i32, idx, f.n), f.q), no_tables=True)[0]
        dense = np.zeros(f.n, dtype=np.int32)
        dense[pos] = i32
        assert f.ctx.msm_indexed_narrow(i32, pos)[0] == f.ctx.run_narrow(dense)[0]
        # bytes with width=, one entry that starts inside a dword (device-side alignment handling of the 1-byte form)
        got, _ = f.ctx.msm_indexed_narrow(u8.tobytes(), idx, width=1)
        assert f.point(got) == f.dlog(idx, u8.tolist())
        assert f.point(f.ctx.msm_indexed_narrow(np.zeros(0, dtype=np.int16), np.zeros(0, dtype=np.uint32))[0]) == f.cv.zero
    finally:
        f.ctx.close()


def test_narrow_value_outside_the_declared_range(f13):
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmError

    f = f13
    vals = np.full(100, 5, dtype=np.uint64)
    idx = np.arange(100, dtype=np.uint32)
    for at in (0, 50, 99):
        bad = vals.copy()
        bad[at] = 1 << 40
        with pytest.raises(MsmError) as e:
            f.ctx.msm_indexed_narrow(bad, idx, bits=40)
        assert e.value.code == _lib.MSM_ERR_SCALAR
    neg = np.full(100, -3, dtype=np.int32)
    neg[7] = -(1 << 16) - 1
    with pytest.raises(MsmError) as e:
        f.ctx.msm_indexed_narrow(neg, idx, bits=16)
    assert e.value.code == _lib.MSM_ERR_SCALAR
    got, _ = f.ctx.msm_indexed_narrow(vals, idx, bits=40)                  # the context goes on working
    assert f.point(got) == f.dlog(idx, vals.tolist())
    for kw in ({"width": 3}, {"width": 8, "bits": 65}, {"width": 32}):     # what msm_run_narrow refuses
        with pytest.raises(MsmError) as e:
            f.ctx.msm_indexed_narrow(bytes(96), list(range(96 // kw["width"])), **kw)
        assert e.value.code == _lib.MSM_ERR_ARG, kw


# ---------------------------------------------------------------------------------------------- 10: refusals

def test_out_of_range_index_names_the_smallest_bad_position(f7):
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmError

    f, m = f7, 1001                                     # (not a multiple of 4: the tail of the check's 16-byte loads)
    good = np.asarray(_ints(f"{f.name}/bad/i", m, f.n), dtype=np.uint32)
    sc = _ints(f"{f.name}/bad/s", m, f.q)
    raw = O.scalars_to_bytes(sc)
    for at, value in ((0, f.n), (m // 2, f.n + 17), (m - 1, (1 << 32) - 1), (m - 2, 1 << 31), (3, f.n)):
        idx = good.copy()
        idx[at] = value
        with pytest.raises(MsmError) as e:
            f.ctx.msm_indexed(raw, idx)
        assert e.value.code == _lib.MSM_ERR_ARG
        assert f"indices[{at}] = {value}" in str(e.value) and f"{f.n} resident" in str(e.value), str(e.value)
        f.check(good, sc)                                # the next valid call on the same context succeeds
    idx = good.copy()
    idx[[900, 333, 334, 1000]] = (f.n, f.n + 1, f.n + 2, f.n + 3)      # the smallest bad position is the one reported
    with pytest.raises(MsmError) as e:
        f.ctx.msm_indexed(raw, idx)
    assert f"indices[333] = {f.n + 1}" in str(e.value)
    with pytest.raises(MsmError) as e:
        f.ctx.msm_indexed_narrow(np.ones(m, dtype=np.uint8), idx)
    assert e.value.code == _lib.MSM_ERR_ARG and f"indices[333] = {f.n + 1}" in str(e.value)
    with pytest.raises(MsmError) as e:                                  # one entry, and it is bad
        f.ctx.msm_indexed(raw[:32], [f.n])
    assert f"indices[0] = {f.n}" in str(e.value)
    assert f.ctx.n_points == f.n and f.ctx.get_point(f.n - 1) == f.cv.scale_g(f.logs[f.n - 1])   # the point set is untouched


def test_refused_options_and_arguments(f13):
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmContext, MsmError
    from montgomery_amd._lib import MsmOpts, MsmResult

    f, m = f13, 64
    lib, h = f.ctx._lib, f.ctx._h
    raw = (ctypes.c_uint8 * (32 * m)).from_buffer_copy(O.scalars_to_bytes(_ints("opts/s", m, f.q)))
    small = (ctypes.c_uint8 * m)(*([1] * m))
    idx = (ctypes.c_uint32 * m)(*range(m))
    res = MsmResult()

    def wide(opts, s=raw, i=idx, n=m, r=res):
        return lib.msm_run_indexed(h, s, i, n, 0, ctypes.byref(opts) if opts is not None else None, ctypes.byref(r) if r is not None else None)

    def narrow(opts, s=small, i=idx, n=m, r=res):
        return lib.msm_run_indexed_narrow(h, s, i, n, 0, 1, 0, 0, ctypes.byref(opts) if opts is not None else None,
                                          ctypes.byref(r) if r is not None else None)

    assert wide(None) == _lib.MSM_OK and narrow(None) == _lib.MSM_OK and wide(MsmOpts(unsafe=1, no_tables=1)) == _lib.MSM_OK
    for bad in (MsmOpts(point_lo=1), MsmOpts(k_lo=0, k_hi=2), MsmOpts(k_lo=1, k_hi=2), MsmOpts(bucket_shards=2),
                MsmOpts(bucket_shards=2, bucket_shard=1), MsmOpts(merged_sums=1), MsmOpts(by_window=1), MsmOpts(c=1), MsmOpts(c=25)):
        assert wide(bad) == _lib.MSM_ERR_ARG, [getattr(bad, n) for n, _ in MsmOpts._fields_]
        assert narrow(bad) == _lib.MSM_ERR_ARG, [getattr(bad, n) for n, _ in MsmOpts._fields_]
    for call in (wide, narrow):
        assert call(None, s=None) == _lib.MSM_ERR_ARG        # null pointers with m > 0
        assert call(None, i=None) == _lib.MSM_ERR_ARG
        assert call(None, r=None) == _lib.MSM_ERR_ARG
        assert call(None, n=1 << 30) == _lib.MSM_ERR_ARG
        assert call(None, s=None, i=None, n=0) == _lib.MSM_OK and (res.is_infinity == 1)
    assert wide(MsmOpts()) == _lib.MSM_OK                     # still usable
    # device indices that are not 4-byte aligned
    dev = f.ctx.device_alloc(32 * m + 4 * m + 64)
    try:
        f.ctx.device_upload(dev, bytes(raw) + bytes(idx))
        r = lib.msm_run_indexed(h, ctypes.c_void_p(dev), ctypes.cast(ctypes.c_void_p(dev + 32 * m + 2), ctypes.POINTER(ctypes.c_uint32)), m - 1, 1,
                                None, ctypes.byref(res))
        assert r == _lib.MSM_ERR_ARG
    finally:
        f.ctx.device_free(dev)
    # strict: a scalar >= q
    sc = _ints("strict/s", m, f.q)
    ok = O.scalars_to_bytes(sc)
    over = bytearray(ok)
    over[32 * 9:32 * 10] = (f.q + 5).to_bytes(32, "little")
    ii = np.arange(m, dtype=np.uint32)
    with pytest.raises(MsmError) as e:
        f.ctx.msm_indexed(bytes(over), ii, strict=True)
    assert e.value.code == _lib.MSM_ERR_SCALAR
    assert f.ctx.msm_indexed(ok, ii, strict=True)[0] == f.ctx.msm_indexed(ok, ii)[0]
    sc[9] = 5                                                 # default: q + 5 is reduced mod q
    assert f.point(f.ctx.msm_indexed(bytes(over), ii)[0]) == f.dlog(ii, sc)
    # no points yet; a device-list context
    empty = MsmContext(f.cv.cid)
    try:
        for call in (lambda: empty.msm_indexed(ok, ii), lambda: empty.msm_indexed_narrow(np.ones(m, dtype=np.uint8), ii)):
            with pytest.raises(MsmError) as e:
                call()
            assert e.value.code == _lib.MSM_ERR_NO_POINTS
    finally:
        empty.close()
    multi = MsmContext(f.cv.cid, devices=[0, 0])
    try:
        multi.generate_points(256, seed=3)
        for call in (lambda: multi.msm_indexed(ok, ii), lambda: multi.msm_indexed_narrow(np.ones(m, dtype=np.uint8), ii)):
            with pytest.raises(MsmError) as e:
                call()
            assert e.value.code == _lib.MSM_ERR_ARG
    finally:
        multi.close()


# ---------------------------------------------------------------------------------------------- 11: window tables stay

def test_window_tables_are_untouched(f13):
    f, m = f13, 2000
    try:
        assert f.ctx.precompute()[1] > 0, "no window tables at 2^13 points"
        before = (f.ctx.tables_info(), f.ctx.tables_range())
        dense_sc = O.scalars_to_bytes(_ints("tab/d", f.n, f.q))
        ref, info = f.ctx.run(dense_sc)
        assert info["tables"]
        idx = _ints("tab/i", m, f.n)
        sc = _ints("tab/s", m, f.q)
        for kw in ({}, {"c": before[0][0]}, {"c": 21}):
            _, ii = f.check(idx, sc, **kw)
            assert not ii["tables"]
            assert (f.ctx.tables_info(), f.ctx.tables_range()) == before
        f.ctx.msm_indexed_narrow(np.ones(m, dtype=np.uint16), np.asarray(idx, dtype=np.uint32))
        assert (f.ctx.tables_info(), f.ctx.tables_range()) == before
        again, info = f.ctx.run(dense_sc)
        assert info["tables"] and again == ref
    finally:
        f.ctx.generate_points(f.n, seed=1302)              # the fixture's points again, without tables


# ---------------------------------------------------------------------------------------------- 12: device input

@pytest.mark.parametrize("m", [1, 1000, 4099])
def test_device_inputs_equal_host_inputs(f13, m):
    f = f13
    idx = np.asarray(_ints(f"dev/{m}/i", m, f.n), dtype=np.uint32)
    sc = _ints(f"dev/{m}/s", m, f.q)
    raw = O.scalars_to_bytes(sc)
    host, _ = f.check(idx, sc)
    vals = np.asarray(_ints(f"dev/{m}/v", m, 1 << 16), dtype=np.uint16)
    host_n, _ = f.ctx.msm_indexed_narrow(vals, idx)
    d_s, d_i, d_v = f.ctx.device_alloc(32 * m), f.ctx.device_alloc(4 * m + 16), f.ctx.device_alloc(2 * m + 16)
    try:
        f.ctx.device_upload(d_s, raw)
        f.ctx.device_upload(d_i, bytes(4) + idx.tobytes())     # indices that start 4 bytes into the buffer: not 16-byte aligned
        f.ctx.device_upload(d_v, vals.tobytes())
        assert f.ctx.msm_indexed_device(d_s, d_i + 4, m)[0] == host
        assert f.ctx.msm_indexed_device(d_s, d_i + 4, m, c=18)[0] == host
        assert f.ctx.msm_indexed_narrow_device(d_v, d_i + 4, m, 2)[0] == host_n
    finally:
        for p in (d_s, d_i, d_v):
            f.ctx.device_free(p)


def test_facade_in_the_shape_of_the_reference():
    """`Curve.Parallel.msmIndexed` / `msmIndexedNarrow` next to `msm`, and sparse_from_dense feeding them."""
    from montgomery_amd import api, narrow

    cv = api.Weierstrass.create(api.PALLAS_PARAMS)
    try:
        par, n = cv.Parallel, 500
        pp = par.randomPointsFast(n, seed=12)
        sc = _ints("facade/s", n, api.PALLAS_PARAMS.order)
        keep = _ints("facade/k", n, 4)
        dense = O.scalars_to_bytes([s if k == 0 else 0 for s, k in zip(sc, keep)])
        idx, nz = api.sparse_from_dense(dense)
        assert 0 < idx.size < n
        sp = par.getScalarPointer(len(dense))
        par.scalarsFromBytes(sp, dense, n)
        exp = par.msm(sp, pp, n)["result"]
        assert par.msmIndexed(nz, idx, pp)["result"] == exp
        assert par.msmIndexed(nz, idx, pp, {"c": 9, "noGlv": True})["result"] == exp
        col = np.zeros(n, dtype=np.int16)
        col[::7] = -3
        col[3::11] = 300
        par.scalarsFromBytes(sp, narrow.widen(col, api.PALLAS_PARAMS.order), n)
        i2, nz2 = api.sparse_from_dense(col)
        assert par.msmIndexedNarrow(nz2, i2, pp)["result"] == par.msm(sp, pp, n)["result"]
    finally:
        cv.context.close()
