"""Round 1 of the accumulation tree in its pair form -- k_bin_pairs' tile-ordered pairs, k_batch_add<MODE_GATHER> writing every
sum to dest[e] as 64-byte element records, round 2 reading the records back -- at sizes of a few seconds.

At the default threshold the pair form needs more than 2^23 table rows, so the suite reached it with BLS12-377 at c = 18 and with
random scalars from 2^24 points only.  msm_test_set_chunk_rows_log lowers the threshold of a context; the pipeline's own host
code then takes the pair form wherever the rest of its rule holds (c >= 18, logG >= 2), and msm_test_last_sort_paths reports what
every window group took.  Every case here

  1. runs under the lowered threshold, asserts from the library's report that ALL its window groups took the pair form, and
     compares the result bit for bit with (sum s_i a_i mod q) G for points of known discrete logs;
  2. runs again in the slot form -- at the default threshold, or a raised one where the case has more than 2^23 rows anyway --
     asserts that no group took the pair form, and that the result is the same.

The sizes are the smallest that give logG >= 2, derived in tests/crafted_digits.py (PAIR_MIN_PLAIN, PAIR_MIN_TABLES) and proven
against its Geometry by tests/test_crafted_digits.py, which also proves, by the bucket walk of the pair form, which kinds of
pair every degenerate layout produces in round 1 and in round 2, bucket by bucket -- in ordinary bins and across the parts of a
heavy one.  Needs an MI355X: `-m gpu`."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import crafted_digits as D
from degenerate_inputs import CURVE_TABLE
from oracle import msm_oracle as O
from test_gpu_sort_shapes import as_c, check_info, expected_point

pytestmark = pytest.mark.gpu

CURVES = ("bls377", "bls381", "pallas", "bn254", "grumpkin", "vesta")
RAISED = 40          # 2^40 rows: no call reaches the pair form


@pytest.fixture(scope="module", params=CURVES)
def cv(request):
    from montgomery_amd.api import MsmContext

    cv = CURVE_TABLE[request.param]
    cv.ctx = MsmContext(cv.cid)
    yield cv
    cv.ctx.close()
    cv.ctx = None


@pytest.fixture(scope="module")
def bn_ctx():
    from montgomery_amd.api import MsmContext

    ctx = MsmContext(CURVE_TABLE["bn254"].cid)
    yield ctx
    ctx.close()


@contextlib.contextmanager
def rows_log(ctx, log2_rows):
    ctx.test_set_chunk_rows_log(log2_rows)
    try:
        yield
    finally:
        ctx.test_set_chunk_rows_log(0)


def in_both_forms(ctx, call, expected, slot_log=0, groups=None):
    """call() -> (result, info) in the pair form and in the slot form (slot_log: 0 = the default threshold).  Returns the info of
    the pair-form run."""
    with rows_log(ctx, D.PAIR_ROWS_LOG):
        res, info = call()
        paths = ctx.test_last_sort_paths()
    print("pair form", paths, {k: info[k] for k in ("c", "K", "tables", "rounds", "max_bucket")})
    assert paths and set(paths) == {"pairs"}, paths
    assert groups is None or len(paths) == groups, paths
    assert res.as_tuple() == expected, info
    with rows_log(ctx, slot_log):
        res2, info2 = call()
        paths2 = ctx.test_last_sort_paths()
    assert len(paths2) == len(paths) and set(paths2) == {"slots"}, paths2
    assert (res2.x, res2.y, res2.isZero) == (res.x, res.y, res.isZero), info2
    assert (info2["c"], info2["K"], info2["tables"], info2["n_pairs_algo"]) == (info["c"], info["K"], info["tables"], info["n_pairs_algo"])
    return info


def uniform(ctx, cv, n, seed, c_oracle):
    """n generated points, n uniform scalars on the device, the expected point."""
    a = ctx.generate_points(n, seed=seed, want_scalars=True, raw=True)
    dev, s = ctx.generate_scalars(n, seed=seed + 1, to_host=True, raw=True)
    return a, dev, s, cv.scale_g(c_oracle.dot_mod(a, s, n, cv.q))


def test_hook_defaults_and_refusals(gpu_ctx, c_oracle):
    """The two test entries themselves: the range of the threshold, rows must EXCEED it, 0 restores the default of 23, the report
    is cut to `cap`, empty after a call that failed or a fused batch, and neither entry serves a device-list context."""
    from montgomery_amd import MsmError
    from montgomery_amd.api import MsmContext

    ctx, lib, h = gpu_ctx, gpu_ctx._lib, gpu_ctx._h
    for bad in (-1, 41):
        with pytest.raises(MsmError):
            ctx.test_set_chunk_rows_log(bad)
    n = D.PAIR_MIN_PLAIN[18]
    a, dev, s, exp = uniform(ctx, CURVE_TABLE["bls377"], n, 2000, c_oracle)
    try:
        # 2^21 rows: more than 2^20, not more than 2^21; 23 set by hand and the default restored by 0 behave alike
        for log2_rows, want in ((20, "pairs"), (21, "slots"), (23, "slots"), (D.PAIR_ROWS_LOG, "pairs"), (0, "slots")):
            ctx.test_set_chunk_rows_log(log2_rows)
            res, info = ctx.run_device(dev, n, c=18, no_tables=True)
            assert ctx.test_last_sort_paths() == [want] and res.as_tuple() == exp, (log2_rows, info)
        # ... and the default is 23: two groups over 2^23 + 4096 rows take the pair form, over 2^23 rows the slot form
        for n_big, want in ((1 << 23, "slots"), ((1 << 23) + 4096, "pairs")):
            ctx.generate_points(n_big, seed=2001)
            dev_big, _ = ctx.generate_scalars(n_big, seed=2002)
            ctx.run_device(dev_big, n_big, c=18, no_tables=True)
            assert ctx.test_last_sort_paths() == [want, want], n_big
        # the report is cut to cap, and its count does not depend on cap
        out = (C.c_int32 * 4)(-7, -7, -7, -7)
        assert lib.msm_test_last_sort_paths(h, out, 1) == 2 and list(out) == [3, -7, -7, -7]
        assert lib.msm_test_last_sort_paths(h, None, 0) == 2 and lib.msm_test_last_sort_paths(None, out, 4) == -1
        assert lib.msm_test_last_sort_paths(h, None, 2) == -1 and lib.msm_test_last_sort_paths(h, out, -1) == -1
        # a call that fails leaves no report behind, nor does a fused batch
        with pytest.raises(MsmError):
            ctx.run_device(dev_big, n_big, c=99)
        assert ctx.test_last_sort_paths() == []
        ctx.generate_points(4096, seed=2003)
        dev_small, _ = ctx.generate_scalars(4096, seed=2004)
        ctx.run_device(dev_small, 4096)
        assert ctx.test_last_sort_paths() == ["one_level"]
        with pytest.raises(MsmError):
            ctx.run_device(dev_small, 4097)                     # more scalars than resident points
        assert ctx.test_last_sort_paths() == [] and lib.msm_test_last_sort_paths(h, None, 0) == 0
        ctx.run_batch_device([dev_small, dev_small], 4096)
        assert ctx.test_last_sort_paths() == []
    finally:
        ctx.test_set_chunk_rows_log(0)
    multi = MsmContext(devices=[0, 0])
    try:
        with pytest.raises(MsmError):
            multi.test_set_chunk_rows_log(10)
        with pytest.raises(MsmError):
            multi.test_last_sort_paths()
        assert multi._lib.msm_test_last_sort_paths(multi._h, None, 0) == -1
    finally:
        multi.close()


# ---------------------------------------------------------------------------------------------- a. every curve

def test_every_curve_plain(cv, c_oracle):
    """2^21 points, c = 18, the plain path: both record layouts (12-word fields: x and y records rec_y_off apart; 8-word fields:
    one record [x | y]) and every instantiation of k_batch_add<CV, MODE_GATHER> with out_rows / dest and with slots == nullptr."""
    n = D.PAIR_MIN_PLAIN[18]
    a, dev, s, exp = uniform(cv.ctx, cv, n, 2100, c_oracle)
    info = in_both_forms(cv.ctx, lambda: cv.ctx.run_device(dev, n, c=18, no_tables=True), exp, groups=1)
    assert (info["c"], info["K"], info["tables"]) == (18, D.Plan(cv.name, 18).K, False)


def test_every_curve_on_window_tables(cv, c_oracle):
    """One merged window of all K 18-bit windows at the smallest n whose mean bucket is 32: 299 594 points (K = 7) or 2^18 (K = 8)."""
    K = D.Plan(cv.name, 18).K
    n = D.PAIR_MIN_TABLES[(18, K)]
    a, dev, s, exp = uniform(cv.ctx, cv, n, 2200, c_oracle)
    cv.ctx.precompute(n, c=18)
    info = in_both_forms(cv.ctx, lambda: cv.ctx.run_device(dev, n, c=18), exp, groups=1)
    assert (info["c"], info["K"], info["tables"]) == (18, K, True)


# ---------------------------------------------------------------------------------------------- b. degenerate pairs

def plant(ctx, cv, dp, seed):
    """Generated points with the rows of dp's groups rewritten (copies, negatives, identities, T): the logs a_i after the edits,
    as an n x 32 byte array, and the points of order 2 planted (their indices)."""
    n = dp.cr.n
    a = np.frombuffer(ctx.generate_points(n, seed=seed, want_scalars=True, raw=True), dtype=np.uint8).reshape(n, 32).copy()
    step = 2 * cv.cb
    wire = np.frombuffer(ctx.get_points(0, n), dtype=np.uint8).reshape(n, step).copy()
    tors = []
    for at, src, sign, t in dp.edits:
        if t:
            wire[at] = np.frombuffer(cv.wire([(cv.p - 1, 0)]), dtype=np.uint8)
            a[at] = 0
            tors.append(at)
        elif src is None:
            wire[at] = 0
            a[at] = 0
        else:
            x = int.from_bytes(wire[src, :cv.cb].tobytes(), "little")
            y = int.from_bytes(wire[src, cv.cb:].tobytes(), "little")
            log = int.from_bytes(a[src].tobytes(), "little")
            wire[at] = np.frombuffer(cv.wire([(x, y if sign > 0 else cv.p - y)]), dtype=np.uint8)
            a[at] = np.frombuffer((sign * log % cv.q).to_bytes(32, "little"), dtype=np.uint8)
    ctx.set_points(wire.tobytes())
    return a, tors


def layouts_case(ctx, cv, c_oracle, dp, call, tables=False, glv=True, seed=2300):
    cr = dp.cr
    a, tors = plant(ctx, cv, dp, seed)
    s = cr.scalars()
    logs = lambda at: int.from_bytes(a[at].tobytes(), "little")     # noqa: E731
    values = dp.values(logs, cv.q)
    for at in tors:
        values[at] = (0, 1)
    D.check_layout_pairs(dp, D.pair_kinds(dp, values, 2, glv=glv))      # with the real logs: the pairs written down for every layout
    exp = cv.scale_g(c_oracle.dot_mod(as_c(a), as_c(s), cr.n, cv.q))
    if tors:        # T is no multiple of G: (sum of its scalars mod 2) T on top
        odd = sum(int.from_bytes(s[at].tobytes(), "little") for at in tors) % 2
        exp = cv.add(exp, (cv.p - 1, 0)) if odd else exp
    if tables:
        ctx.precompute(cr.n, c=cr.plan.c)
    return in_both_forms(ctx, lambda: call(s), exp, groups=1)


@pytest.mark.parametrize("name", ["bls377", "bn254"])
@pytest.mark.parametrize("tables", [False, True], ids=["plain", "tables"])
def test_degenerate_pairs_in_both_rounds(gpu_ctx, bn_ctx, c_oracle, name, tables):
    """The layouts of crafted_digits.DEGENERATE_LAYOUTS, twice each among 2^21 (tables: 299 594) ordinary points: P + P, P - P
    with the identity written as a record, identity rows as either operand and a pair with nothing in round 1; equal, opposite
    and identity records as operands of round 2, BA_COPY_B's second fetch at y_off = rec_y_off (12 words) and 4 NW (8 words)."""
    cv, ctx = CURVE_TABLE[name], (gpu_ctx if name == "bls377" else bn_ctx)
    pl = D.Plan(name, 18)
    n = D.PAIR_MIN_TABLES[(18, pl.K)] if tables else D.PAIR_MIN_PLAIN[18]
    dp = D.degenerate_pairs(pl, n, tables=tables)
    info = layouts_case(ctx, cv, c_oracle, dp, lambda s: ctx.run(as_c(s), c=18, no_tables=not tables), tables=tables)
    assert info["tables"] == tables


@pytest.mark.parametrize("name", ["bls377", "bn254"])
def test_degenerate_pairs_across_the_parts_of_a_heavy_bin(gpu_ctx, bn_ctx, c_oracle, name):
    """The layouts inside a bin that is heavy across the merged window of seven 18-bit windows (crafted_digits.
    degenerate_pairs_in_parts: three parts; every layout's bucket has its entries of window 1 in part 0 and those of window 4 in
    part 1): k_part_scan in elements, part_pair_off and the sub rows of k_bin_pairs with P + P, P - P, identity rows and -- the
    layout of five -- an odd entry paired with nothing at the end of both parts, on the two-record layout of BLS12-377 and on
    the one-record layout [x | y] of BN254."""
    cv, ctx = CURVE_TABLE[name], (gpu_ctx if name == "bls377" else bn_ctx)
    pl = D.Plan(name, 18)
    dp = D.degenerate_pairs_in_parts(pl, D.PAIR_MIN_TABLES[(18, pl.K)])
    info = layouts_case(ctx, cv, c_oracle, dp, lambda s: ctx.run(as_c(s), c=18), tables=True, seed=2350)
    assert info["tables"] and info["max_bucket"] >= 2 * 5


# ---------------------------------------------------------------------------------------------- c. c = 21 and c = 22

@pytest.mark.parametrize("c", [21, 22])
def test_wide_windows_in_the_pair_form(gpu_ctx, c_oracle, c):
    """Six windows as two merged windows of three on window tables, at the smallest n whose mean bucket is 32: 5 592 406 points
    (c = 21), 11 184 811 (c = 22).  Both have more than 2^23 rows, so the slot form is that of a raised threshold."""
    cv = CURVE_TABLE["bls377"]
    n = D.PAIR_MIN_TABLES[(c, 6)]
    a, dev, s, exp = uniform(gpu_ctx, cv, n, 2400 + c, c_oracle)
    gpu_ctx.precompute(n, c=c)
    info = in_both_forms(gpu_ctx, lambda: gpu_ctx.run_device(dev, n, c=c), exp, slot_log=RAISED, groups=2)
    assert (info["c"], info["K"], info["tables"]) == (c, 6, True)


@pytest.mark.parametrize("cs", D.PAIR21_CASES, ids=[cs.id for cs in D.PAIR21_CASES])
def test_heavy_bins_at_c21_in_the_pair_form(gpu_ctx, c_oracle, cs):
    """exact_edges and alternating (an odd entry of every bucket in every part) at c = 21: multi-part bins of 2^11 buckets."""
    cr = cs.make()
    cv = CURVE_TABLE["bls377"]
    a = gpu_ctx.generate_points(cs.n, seed=2500, want_scalars=True, raw=True)
    s = cr.scalars()
    exp = expected_point(c_oracle, cv, a, s, cs.n)
    gpu_ctx.precompute(cs.n, c=cs.c)
    info = in_both_forms(gpu_ctx, lambda: gpu_ctx.run(as_c(s), c=cs.c), exp, slot_log=RAISED, groups=2)
    check_info(cr, info, cs.c, tables=True)


# ---------------------------------------------------------------------------------------------- d. other entry points

def test_narrow_indexed_and_no_glv_on_an_8_word_field(bn_ctx, c_oracle):
    """BN254 G1, 2^21 entries, c = 18: msm_run_narrow (16-byte scalars), msm_run_indexed (a permuted strict subset) and no_glv
    (fifteen windows of the whole scalar in one group)."""
    cv, ctx = CURVE_TABLE["bn254"], bn_ctx
    n, N = D.PAIR_MIN_PLAIN[18], D.PAIR_MIN_PLAIN[18] + 77
    a = ctx.generate_points(N, seed=2600, want_scalars=True, raw=True)
    a_np = np.frombuffer(a, dtype=np.uint8).reshape(N, 32)
    dev, s = ctx.generate_scalars(N, seed=2601, to_host=True, raw=True)
    s_np = np.frombuffer(s, dtype=np.uint8).reshape(N, 32)
    # no_glv over all N points
    exp = cv.scale_g(c_oracle.dot_mod(a, s, N, cv.q))
    info = in_both_forms(ctx, lambda: ctx.run_device(dev, N, c=18, no_glv=True, no_tables=True), exp, groups=1)
    assert info["K"] == -(-(cv.q.bit_length() + 1) // 18)
    # indexed
    idx = np.random.default_rng(26).permutation(N)[:n].astype(np.uint32)
    sel, s_sel = np.ascontiguousarray(a_np[idx]), np.ascontiguousarray(s_np[:n])
    exp = cv.scale_g(c_oracle.dot_mod(as_c(sel), as_c(s_sel), n, cv.q))
    in_both_forms(ctx, lambda: ctx.msm_indexed(s_sel, idx, c=18), exp, groups=1)
    # narrow: the low 16 bytes of the scalars
    wide = np.zeros((N, 32), dtype=np.uint8)
    wide[:, :16] = s_np[:, :16]
    exp = cv.scale_g(c_oracle.dot_mod(a, as_c(wide), N, cv.q))
    narrow = np.ascontiguousarray(wide[:, :16])
    in_both_forms(ctx, lambda: ctx.run_narrow(narrow.tobytes(), signed=False, c=18, width=16), exp, groups=1)


def test_narrow_layouts_with_the_point_of_order_two(gpu_ctx, c_oracle):
    """BLS12-377, msm_run_narrow over crafted 125-bit scalars: the degenerate layouts and, as a narrow call has no endomorphism,
    the point T = (p - 1, 0) of order 2 -- T + T has equal operands with y = 0 and must give the identity record, not a doubling."""
    cv = CURVE_TABLE["bls377"]
    pl = D.Plan("bls377", 18, D.NARROW_BITS)
    dp = D.degenerate_pairs(pl, D.PAIR_MIN_PLAIN[18], layouts=dict(D.DEGENERATE_LAYOUTS, **D.TORSION_LAYOUTS))
    call = lambda s: gpu_ctx.run_narrow(np.ascontiguousarray(s[:, :16]).tobytes(), bits=D.NARROW_BITS, signed=False, c=18, width=16)   # noqa: E731
    layouts_case(gpu_ctx, cv, c_oracle, dp, call, glv=False, seed=2700)


def test_no_glv_with_the_point_of_order_two(gpu_ctx, c_oracle):
    """BLS12-377, no_glv, uniform scalars: T planted at three single places and at FOUR consecutive indices under one scalar.
    Without the endomorphism a point has one entry per window, a bucket's records are in point order and uniform digits leave
    every bin in one part, so in each of the fifteen windows whose digit of that scalar is not zero the four are consecutive
    entries r .. r + 3 of one bucket: round 1 pairs (r, r + 1), (r + 2, r + 3) if r is even and (r + 1, r + 2) if it is odd --
    T + T, equal operands with y = 0, occurs whatever else the bucket holds; the other T meet ordinary points."""
    cv = CURVE_TABLE["bls377"]
    n = D.PAIR_MIN_PLAIN[18]
    a = np.frombuffer(gpu_ctx.generate_points(n, seed=2800, want_scalars=True, raw=True), dtype=np.uint8).reshape(n, 32).copy()
    dev, s = gpu_ctx.generate_scalars(n, seed=2801, to_host=True, raw=True)
    s_np = np.frombuffer(s, dtype=np.uint8).reshape(n, 32).copy()
    wire = np.frombuffer(gpu_ctx.get_points(0, n), dtype=np.uint8).reshape(n, 96).copy()
    places = [3, n // 3, n // 3 + 1, n // 3 + 2, n // 3 + 3, n // 2 + 7, n - 2]
    s_np[n // 3 + 1:n // 3 + 4] = s_np[n // 3]
    assert sum(1 for l, _ in O.signed_digits(int.from_bytes(s_np[n // 3].tobytes(), "little"), 18, 15) if l) >= 8
    for at in places:
        wire[at] = np.frombuffer(cv.wire([(cv.p - 1, 0)]), dtype=np.uint8)
        a[at] = 0
    gpu_ctx.set_points(wire.tobytes())
    exp = cv.scale_g(c_oracle.dot_mod(as_c(a), as_c(s_np), n, cv.q))
    if sum(int.from_bytes(s_np[at].tobytes(), "little") for at in places) % 2:
        exp = cv.add(exp, (cv.p - 1, 0))
    in_both_forms(gpu_ctx, lambda: gpu_ctx.run(as_c(s_np), c=18, no_glv=True, no_tables=True), exp, groups=1)


# ---------------------------------------------------------------------------------------------- e. both forms in one call

def test_both_forms_in_one_call(gpu_ctx, c_oracle):
    """Seven 18-bit windows on window tables run as a group of four and a group of three merged windows: 4 n and 3 n rows.  Only a
    threshold between them splits the forms inside one call, and the row counts differ by a factor of 4 / 3 only, so the
    power of two between them is the default one: 3 n <= 2^23 < 4 n at n = 2^21 + 4096, the smallest size with two groups on
    tables.  (On the plain path every group of a call sees the same n rows: no threshold separates them.)"""
    cv = CURVE_TABLE["bls377"]
    n = D.TABLES_N
    a, dev, s, exp = uniform(gpu_ctx, cv, n, 2900, c_oracle)
    gpu_ctx.precompute(n, c=18)
    got = {}
    for log2_rows in (0, D.PAIR_ROWS_LOG, RAISED):
        with rows_log(gpu_ctx, log2_rows):
            res, info = gpu_ctx.run_device(dev, n, c=18)
            got[log2_rows] = gpu_ctx.test_last_sort_paths()
        assert res.as_tuple() == exp and info["tables"], (log2_rows, info)
    assert got == {0: ["pairs", "slots"], D.PAIR_ROWS_LOG: ["pairs", "pairs"], RAISED: ["slots", "slots"]}, got
