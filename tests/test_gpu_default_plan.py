"""Default-plan calls (c = None) over a RANGE of the resident points, against msm_plan, across the states of the window tables.

On window tables a call may run under another plan than on the plain path (pick_window_tables against pick_window, msm_plan.hip):
BLS12-377, BN254 G1 and Grumpkin take seven folded 18-bit windows instead of eight 16-bit ones from 2^16 points, Ed-on-BLS12-377
14 or 17 bits instead of the cost model's pick.  Which of the two a call gets depends on the state of the context -- the tables that
exist, the tables limit, the range that came back twice.  The contract pinned here (include/msm_hip.h at msm_plan,
msm_window_sums and msm_precompute): msm_plan reports the plan of the very next call and of every call after it over the same
range; only new points, msm_set_tables_limit, msm_precompute and tables of the whole set move it.  A caller sizes its slots and
cuts its window shards from msm_plan's K, and the sums of the ranks of a points split meet slot by slot.

Every result is compared with a host big-integer reference: the points are a_i G with the a_i known, so the MSM over the share
[lo, lo + m) is (sum a_i s_i mod q) G.  Group elements are exact: no tolerances.  The cells are (curve, resident points n,
share m); every call is over the SECOND share (point_lo = m, so the tables of the range do not start at row 0) unless said
otherwise.  Needs an MI355X: `-m gpu`."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import msm_oracle as O  # noqa: E402
from test_cycle_curves import BN254, GRUMPKIN  # noqa: E402

pytestmark = pytest.mark.gpu

SLOT = 144          # bytes of one window sum on the wire
K_MAX = 64          # the library's bound on K (make_plan)
MARK = 0xA5
TABLES_LIMIT = 28 << 30   # what the other table tests restore: the default, 10 % of the device


class Cell:
    """tables / plain: the (c, K) the two paths pick for a share of m points, where the design states them (None: not pinned)."""

    def __init__(self, name, curve, params, lg_n, lg_m, tables=None, plain=None):
        self.name, self.curve, self.B = name, curve, params
        self.n, self.m = 1 << lg_n, 1 << lg_m
        self.tables, self.plain = tables, plain
        self.te = isinstance(params, O.TwistedEdwardsParams)
        self.seed = 7000 + 100 * curve + lg_m

    def point(self, k):
        """k G as the affine pair the results are compared with"""
        B = self.B
        if self.te:
            return O.te_to_affine(O.te_scale(k % B.q, O.te_from_affine((B.gx, B.gy), B), B), B)
        return O.aff_scale(k % B.q, (B.gx, B.gy), B.p)

    def xy(self, res):
        return (res.x, res.y) if self.te else res.as_tuple()

    def identity(self, part, j):
        """slot j of `part` holds the identity: Z = 0 (projective), or X = 0 and Y = Z (extended Edwards without T)"""
        X, Y, Z = (int.from_bytes(part[SLOT * j + 48 * i: SLOT * j + 48 * i + 48], "little") for i in range(3))
        return (X == 0 and Y == Z and Z != 0) if self.te else Z == 0


# curve ids: montgomery_amd/_lib.py (0 BLS12-377 G1, 1 Ed-on-BLS12-377, 2 BLS12-381 G1, 3 Pallas, 4 BN254 G1, 5 Grumpkin)
CELLS = [
    Cell("bls377-2p16", 0, O.BLS12_377, 17, 16, tables=(18, 7), plain=(16, 8)),
    Cell("bn254-2p16", 4, BN254, 17, 16, tables=(18, 7), plain=(16, 8)),          # the same rule on the 9-limb field
    Cell("grumpkin-2p16", 5, GRUMPKIN, 17, 16, tables=(18, 7), plain=(16, 8)),
    Cell("ed377-2p14", 1, O.ED_ON_BLS12_377, 15, 14, tables=(14, 18), plain=(9, 28)),
    Cell("ed377-2p17", 1, O.ED_ON_BLS12_377, 18, 17, tables=(17, 15)),
    Cell("bls377-2p14", 0, O.BLS12_377, 15, 14, tables=(16, 8), plain=(16, 8)),   # control: both picks 16
    Cell("bls381-2p16", 2, O.BLS12_381, 17, 16, tables=(16, 8), plain=(16, 8)),   # control: the tables pick is the plain pick
    Cell("pallas-2p16", 3, O.PALLAS, 17, 16, tables=(16, 8), plain=(16, 8)),      # control: the same on the 9-limb field
]


@pytest.fixture(scope="module")
def contexts(gpu_ctx):
    """One context per curve for the module; BLS12-377 is the session's."""
    from montgomery_amd.api import MsmContext

    made = {0: gpu_ctx}

    def get(curve):
        if curve not in made:
            made[curve] = MsmContext(curve)
        return made[curve]

    yield get
    for curve, ctx in made.items():
        if curve != 0:
            ctx.close()
    gpu_ctx.set_tables_limit(TABLES_LIMIT)


@pytest.fixture(params=CELLS, ids=[c.name for c in CELLS])
def cell(request):
    return request.param


_REFERENCES = {}   # (cell name, n, m) -> {point_lo: expected point}: computed once, shared by the tests, never changed


def view(arr, first, count):
    """scalars [first, first + count) of a ctypes array of 32-byte scalars, not copied"""
    return (C.c_uint8 * (32 * count)).from_buffer(arr, 32 * first)


class State:
    """Fresh state of a cell: n new resident points (which drops every table and the remembered range), n device scalars, and
    the expected sums over [0, m), [m, 2m) and the whole set.  The same seeds every time: the references are computed once."""

    def __init__(self, ctx, cl, c_oracle, n=None, m=None):
        self.ctx, self.cl = ctx, cl
        self.n, self.m = n or cl.n, m or cl.m
        n, m = self.n, self.m
        a = ctx.generate_points(n, seed=cl.seed, want_scalars=True, raw=True)
        self.dev, s = ctx.generate_scalars(n, seed=cl.seed + 1, to_host=True, raw=True)
        key = (cl.name, n, m)
        if key not in _REFERENCES:
            q = cl.B.q
            ref = {lo: c_oracle.dot_mod(view(a, lo, m), view(s, lo, m), m, q) for lo in (0, m)}
            ref["whole"] = c_oracle.dot_mod(a, s, n, q)
            _REFERENCES[key] = {k: cl.point(v) for k, v in ref.items()}
        self.exp = _REFERENCES[key]
        assert ctx.tables_info() == (0, 0, 0) and ctx.tables_range() == (0, 0)

    def plan(self, lo):
        return self.ctx.plan(self.m, merged=True, point_lo=lo)

    def sums(self, lo, K):
        """window_sums(merged) over the share at lo, default plan, all K windows"""
        return self.ctx.window_sums(self.dev + 32 * lo, self.m, 0, K, on_device=True, point_lo=lo, merged=True)

    def combine(self, part, K, c):
        from montgomery_amd.distributed import combine_groups_host

        return combine_groups_host(part, 1, K, c, self.ctx.curve)

    def checked_call(self, lo, tables=None):
        """msm_plan, then the call it describes: the plan is the call's, the sum is the reference's.  -> (plan, part, info)"""
        p = self.plan(lo)
        part, info = self.sums(lo, p[1])
        assert (info["c"], info["K"]) == p, (self.cl.name, lo, p, info)
        assert self.combine(part, p[1], p[0]) == self.exp[lo], (self.cl.name, lo, p, info)
        if tables is not None:
            assert info["tables"] == tables, (self.cl.name, lo, p, info)
        return p, part, info


@pytest.fixture
def state(contexts, cell, c_oracle):
    ctx = contexts(cell.curve)
    ctx.set_tables_limit(TABLES_LIMIT)
    return State(ctx, cell, c_oracle)


def test_plan_equals_call_and_stays_put(state, cell):
    """(a) msm_plan before each of three calls in a row over one range: one plan, every call reports it and sums to the reference.
    The first call builds nothing (a caller walking over shards must be spared the build), the second and third run on the
    tables of the range."""
    ctx, m = state.ctx, state.m
    p = state.plan(m)
    print(cell.name, "plan", p, "plain plan", ctx.plan(m, no_tables=True))
    if cell.tables:
        assert p == cell.tables
    if cell.plain:
        assert ctx.plan(m, no_tables=True) == cell.plain
    for call in (1, 2, 3):
        assert state.plan(m) == p, (cell.name, call)
        part, info = state.sums(m, p[1])
        print(cell.name, "call", call, "ran", (info["c"], info["K"]), "tables", info["tables"])
        assert (info["c"], info["K"]) == p, (cell.name, call, info)
        assert state.combine(part, p[1], p[0]) == state.exp[m], (cell.name, call, info)
        if call == 1:
            assert not info["tables"] and ctx.tables_info() == (0, 0, 0)
        else:
            assert info["tables"] and ctx.tables_info()[:2] == p and ctx.tables_range() == (m, m), (cell.name, call)
        if call == 2:
            assert not cell.identity(part, 0) and all(cell.identity(part, j) for j in range(1, p[1]))
        assert state.plan(m) == p, (cell.name, call)


def raw_window_sums(ctx, dev, m, lo, k_lo=0, k_hi=0):
    """msm_window_sums through the C ABI, default plan, merged_sums, into a buffer of K_MAX slots prefilled with MARK: a wrong
    slot count lands in memory the test owns.  -> (buffer as bytes, msm_result)"""
    from montgomery_amd import _lib

    buf = (C.c_uint8 * (K_MAX * SLOT))()
    C.memset(buf, MARK, K_MAX * SLOT)
    opts = _lib.MsmOpts(c=0, k_lo=k_lo, k_hi=k_hi, point_lo=lo, merged_sums=1)
    res = _lib.MsmResult()
    rc = ctx._lib.msm_window_sums(ctx._h, C.c_void_p(dev + 32 * lo), m, 1, C.byref(opts), buf, C.byref(res))
    assert rc == _lib.MSM_OK, ctx._lib.msm_last_error(ctx._h)
    return bytes(buf), res


def test_slot_count_through_the_raw_abi(state, cell):
    """(b) k_lo = k_hi = 0 asks for all windows: the call writes msm_plan's K slots and not a byte more -- on a fresh range, once
    more, and for a window shard cut from the reported plan (on the tables, and on the plain path of a range seen first)."""
    ctx, m, dev = state.ctx, state.m, state.dev
    untouched = bytes([MARK])
    for call in (1, 2):
        c, K = state.plan(m)
        out, res = raw_window_sums(ctx, dev, m, m)
        written = len(out.rstrip(untouched))
        print(cell.name, "call", call, "plan", (c, K), "ran", (res.c, res.K), "bytes written <=", written)
        assert res.K == K and res.c == c, (cell.name, call, (c, K), (res.c, res.K))
        assert out[SLOT * K:] == untouched * (SLOT * (K_MAX - K)), (cell.name, call, K, written)
        assert state.combine(out[: SLOT * K], K, c) == state.exp[m], (cell.name, call)
        assert bool(res.tables) == (call == 2)
    # windows [2, 5) of the reported plan: three slots, which take the place of slots 2 .. 4 of one P_k per slot (the plain path
    # under the same window); lo = m: on the tables of the range; lo = 0: a range seen for the first time
    k_lo, k_hi = 2, 5
    for lo in (m, 0):
        c, K = state.plan(lo)
        assert k_hi <= K
        out, res = raw_window_sums(ctx, dev, m, lo, k_lo, k_hi)
        assert (res.c, res.K) == (c, K), (cell.name, lo, (c, K), (res.c, res.K))
        assert out[SLOT * (k_hi - k_lo):] == untouched * (SLOT * (K_MAX - (k_hi - k_lo))), (cell.name, lo)
        assert bool(res.tables) == (lo == m)
        ref, _ = ctx.window_sums(dev + 32 * lo, m, 0, K, c=c, on_device=True, point_lo=lo)
        assert state.combine(ref, K, c) == state.exp[lo]
        mixed = ref[: SLOT * k_lo] + out[: SLOT * (k_hi - k_lo)] + ref[SLOT * k_hi:]
        assert state.combine(mixed, K, c) == state.exp[lo], (cell.name, lo)


def test_another_range_while_range_tables_exist(state, cell):
    """(c) the tables of [m, 2m) exist; [0, m) comes twice under one plan and takes the tables over; the first range is still right."""
    ctx, m = state.ctx, state.m
    for call in (1, 2, 3):
        state.checked_call(m, tables=call > 1)
    assert ctx.tables_range() == (m, m)
    p0 = state.plan(0)
    for call in (1, 2):
        p, _, info = state.checked_call(0, tables=call > 1)
        assert p == p0, (cell.name, call, p, p0)
    assert ctx.tables_range() == (0, m) and ctx.tables_info()[:2] == p0
    state.checked_call(m, tables=False)
    assert ctx.tables_range() == (0, m)


def test_msm_run_over_the_range(state, cell):
    """(d) msm_run over the range, default plan, three times: one (c, K) -- msm_plan's for the range -- and the reference every
    time; the plain path beside it as a second witness.  (On BLS12-377 and BN254 these are the suite's runs of folded 18-bit
    tables of a range against an independent reference.)"""
    ctx, m, dev = state.ctx, state.m, state.dev
    p = state.plan(m)
    seen = []
    for call in (1, 2, 3):
        res, info = ctx.run_device(dev + 32 * m, m, point_lo=m)
        print(cell.name, "msm_run", call, "ran", (info["c"], info["K"]), "tables", info["tables"])
        seen.append((info["c"], info["K"]))
        assert cell.xy(res) == state.exp[m], (cell.name, call, info)
        if info["tables"]:
            assert ctx.tables_info()[:2] == (info["c"], info["K"]) and ctx.tables_range() == (m, m)
        assert info["tables"] == (call > 1), (cell.name, call, info)
    assert seen == [p] * 3, (cell.name, p, seen)
    plain, ip = ctx.run_device(dev + 32 * m, m, point_lo=m, no_tables=True)
    assert not ip["tables"] and cell.xy(plain) == state.exp[m], ip
    assert (ip["c"], ip["K"]) == ctx.plan(m, no_tables=True)
    whole, _ = ctx.run_device(dev, state.n, no_tables=True)
    assert cell.xy(whole) == state.exp["whole"]


def test_state_changes_that_move_the_plan(state, cell, c_oracle):
    """(e) what may legitimately move the plan: after each act msm_plan and the very next call agree, and the sum is right."""
    ctx, n, m, dev = state.ctx, state.n, state.m, state.dev
    tables_plan, plain_plan = state.plan(m), ctx.plan(m, no_tables=True)
    # no tables allowed: the plain plan, and nothing is built however often the range comes back
    ctx.set_tables_limit(0)
    try:
        for call in (1, 2):
            p, _, _ = state.checked_call(m, tables=False)
            assert p == plain_plan and ctx.tables_info() == (0, 0, 0), (cell.name, call, p)
    finally:
        ctx.set_tables_limit(TABLES_LIMIT)
    # msm_precompute of the range, default window: the tables are there before the first call, which runs on them
    c, K, nbytes = ctx.precompute(m, point_lo=m)
    assert (c, K) == tables_plan and nbytes > 0 and ctx.tables_range() == (m, m)
    for call in (1, 2):
        p, part, _ = state.checked_call(m, tables=True)
        assert p == tables_plan and all(cell.identity(part, j) for j in range(1, K))
    # tables of the whole set replace them and stay: calls over the range run, and msm_plan reports, the plain plan
    whole, iw = ctx.run_device(dev, n)
    assert iw["tables"] and (iw["c"], iw["K"]) == ctx.plan(n) and cell.xy(whole) == state.exp["whole"], iw
    assert ctx.tables_range() == (0, n)
    for call in (1, 2):
        p, _, _ = state.checked_call(m, tables=False)
        assert p == plain_plan and ctx.tables_range() == (0, n), (cell.name, call, p)
    res, info = ctx.run_device(dev + 32 * m, m, point_lo=m)
    assert cell.xy(res) == state.exp[m] and (info["c"], info["K"]) == plain_plan and not info["tables"], info
    # new points (the same ones: the references hold) drop everything
    fresh = State(ctx, cell, c_oracle)
    assert fresh.plan(m) == tables_plan
    fresh.checked_call(m, tables=False)
    assert ctx.tables_info() == (0, 0, 0)
    fresh.checked_call(m, tables=True)


# the bounds of eligibility: a call over fewer than 4096 points never runs on tables; 2^16 - 1 points on BLS12-377 are the last
# size whose tables pick is still 16 bits
BLS377, ED377 = CELLS[0], CELLS[3]
EDGES = [(BLS377, 4095), (BLS377, 4096), (BLS377, (1 << 16) - 1), (ED377, 4095), (ED377, 4096)]


@pytest.mark.parametrize("cl,m", EDGES, ids=[f"{c.name.split('-')[0]}-{m}" for c, m in EDGES])
def test_bounds_of_eligibility(contexts, c_oracle, cl, m):
    """(f) plan = call = reference on calls 1 and 2 over the second of two shares of m points."""
    ctx = contexts(cl.curve)
    ctx.set_tables_limit(TABLES_LIMIT)
    st = State(ctx, cl, c_oracle, n=2 * m, m=m)
    plans = []
    for call in (1, 2):
        p, _, info = st.checked_call(m, tables=(call == 2 and m >= 4096))
        print(cl.name, m, "call", call, "plan", p, "tables", info["tables"])
        plans.append(p)
    assert plans[0] == plans[1], (cl.name, m, plans)
    if not cl.te and m == (1 << 16) - 1:
        assert plans[0] == (16, 8)
