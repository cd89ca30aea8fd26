"""The resident sumcheck on the GPU: msm_scalars_sumcheck_round, msm_scalars_bind and msm_scalars_eq.  `-m gpu`.

Expected values are Python integers mod cv.q; every comparison is bit-exact.  Tables sit at an odd 32-byte offset inside their
allocation, end in a sentinel element, and carry non-canonical elements (q, q + 1, 2^256 - 1) and zeros among the random ones.
Sizes: 1, 2, 32, 64, 128, 256 and 512 pairs -- below a wave, one wave, one block, two blocks -- and 1024 pairs under a forced
grid of one block (four pairs per lane) and of three (a ragged second stride)."""
import ctypes
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degenerate_inputs as D  # noqa: E402
import operator_fixture as F  # noqa: E402
from operator_fixture import SENTINEL, TOP, OperatorFixture, to_bytes  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = (("prod", 1), ("prod", 2), ("prod", 3), ("prod", 4), ("r1cs", 4))
ROUND_LOGS = (1, 2, 6, 7, 8, 9, 10)
NLOG = 10
N = 1 << NLOG


def _ints(tag, n, bound):
    return O.prng_ints(f"sumcheck/{tag}", n, bound)


mixed = functools.partial(F.mixed, "sumcheck")


def lo_of(i, var):
    return ((i >> var) << (var + 1)) | (i & ((1 << var) - 1))


def degree(shape, m):
    return 3 if shape == "r1cs" else m


def g_of(shape, f, q):
    if shape == "r1cs":
        return f[0] * (f[1] * f[2] - f[3]) % q
    p = 1
    for x in f:
        p = p * x % q
    return p


def round_ref(tables, log2n, var, shape, q):
    """s(0 .. d) over the first 2^log2n elements of each table"""
    h, m = 1 << (log2n - 1), len(tables)
    out = [0] * (degree(shape, m) + 1)
    for i in range(h):
        lo = lo_of(i, var)
        hi = lo + (1 << var)
        for t in range(len(out)):
            out[t] += g_of(shape, [a[lo] + t * (a[hi] - a[lo]) for a in tables], q)
    return [x % q for x in out]


def bind_ref(a, log2n, var, r, q):
    return [(a[lo_of(i, var)] + r * (a[lo_of(i, var) + (1 << var)] - a[lo_of(i, var)])) % q for i in range(1 << (log2n - 1))]


def eq_ref(point, s, q):
    tab = [s % q]
    for r in point:                                  # variable j doubles the table: bit j of the index
        tab = [x * (1 - r) % q for x in tab] + [x * r % q for x in tab]
    return tab


def interpolate(evals, x, q):
    """the value at x of the polynomial of degree len(evals) - 1 through (t, evals[t])"""
    total = 0
    for t, y in enumerate(evals):
        num = den = 1
        for u in range(len(evals)):
            if u != t:
                num = num * (x - u) % q
                den = den * (t - u) % q
        total += y * num * pow(den, -1, q)
    return total % q


class Fix(OperatorFixture):
    def __init__(self, name):
        super().__init__(name)
        self._tables = None

    def tables(self):
        """eight tables of 2^10 mixed elements, uploaded once and only ever read: (values, device addresses)"""
        if self._tables is None:
            vals = [mixed(self.cv, f"tab/{j}", N) for j in range(8)]
            self._tables = (vals, [self.vector(v, pad=3 + 2 * (j % 2)) for j, v in enumerate(vals)])
        return self._tables

    def last(self):
        out = super().last("msm_test_last_sumcheck", 4)
        assert len(out) == 4
        return out

    def set_grid(self, blocks):
        self.set("msm_test_set_sumcheck_grid", blocks)


@pytest.fixture(scope="module", params=D.NAMES)
def f7(request):
    f = Fix(request.param)
    yield f
    f.close()


# ---------------------------------------------------------------------------------------------- 1: the round

def test_round_every_shape_at_every_size(f7):
    f, q, ctx = f7, f7.q, f7.ctx
    vals, ptrs = f.tables()
    for log2n in ROUND_LOGS:
        for var in sorted({log2n // 2, log2n - 1}):
            for shape, m in SHAPES:
                got = ctx.scalars_sumcheck_round(ptrs[:m], log2n, var, shape)
                assert got == round_ref(vals[:m], log2n, var, shape, q), (f.name, log2n, var, shape, m)
                assert f.last()[:3] == [max(1, (1 << (log2n - 1)) // 256), 1 << (log2n - 1), degree(shape, m) + 1]
    for j in range(4):
        assert f.read(ptrs[j], N) == vals[j] and f.is_sentinel(ptrs[j] - 32) and f.is_sentinel(ptrs[j] + 32 * N)


def test_round_every_variable_and_shared_vectors(f7):
    f, q, ctx = f7, f7.q, f7.ctx
    vals, ptrs = f.tables()
    for log2n in (3, NLOG):
        for var in range(log2n):
            assert ctx.scalars_sumcheck_round(ptrs[:2], log2n, var) == round_ref(vals[:2], log2n, var, "prod", q), (f.name, log2n, var)
    # the same pointer twice, and two vectors one element apart
    assert ctx.scalars_sumcheck_round([ptrs[0], ptrs[0]], NLOG, 4) == round_ref([vals[0], vals[0]], NLOG, 4, "prod", q)
    assert ctx.scalars_sumcheck_round([ptrs[1], ptrs[1] + 32, ptrs[1]], 9, 8) == \
        round_ref([vals[1], vals[1][1:], vals[1]], 9, 8, "prod", q)
    # s(0) + s(1) is the sum of g over the whole table, whichever variable is bound
    total = sum(a * b for a, b in zip(vals[0], vals[1])) % q
    assert total == ctx.scalars_inner(ptrs[0], ptrs[1], N)
    for var in (0, 5, 9):
        s = ctx.scalars_sumcheck_round(ptrs[:2], NLOG, var)
        assert (s[0] + s[1]) % q == total


def test_round_results_do_not_depend_on_the_grid(f7):
    f, q, ctx = f7, f7.q, f7.ctx
    log2n, n = 11, 1 << 11
    V = [mixed(f.cv, f"grid/{j}", n) for j in range(4)]
    ptrs = [f.vector(v) for v in V]
    try:
        for shape, m in (("prod", 2), ("prod", 4), ("r1cs", 4)):
            for var in (10, 3):
                exp = round_ref(V[:m], log2n, var, shape, q)
                f.set_grid(0)
                assert ctx.scalars_sumcheck_round(ptrs[:m], log2n, var, shape) == exp
                assert f.last()[:3] == [4, 1024, len(exp)]
                for blocks in (1, 3):                       # four pairs per lane; a second stride of 256 of 768 lanes
                    f.set_grid(blocks)
                    assert ctx.scalars_sumcheck_round(ptrs[:m], log2n, var, shape) == exp, (f.name, shape, m, var, blocks)
                    assert f.last()[:3] == [blocks, 1024, len(exp)]
    finally:
        f.set_grid(0)
    assert ctx._lib.msm_test_set_sumcheck_grid(ctx._h, 1025) != 0 and ctx._lib.msm_test_set_sumcheck_grid(ctx._h, -1) != 0
    assert ctx.scalars_sumcheck_round(ptrs[:2], log2n, 0) == round_ref(V[:2], log2n, 0, "prod", q)
    assert f.last()[0] == 4


# ---------------------------------------------------------------------------------------------- 2: bind

def test_bind_every_variable_one_and_eight_vectors(f7):
    f, q, ctx = f7, f7.q, f7.ctx
    vals, ptrs = f.tables()
    dsts = [f.vector(N // 2, pad=1 + 2 * (j % 2)) for j in range(8)]
    rs = _ints(f"{f.name}/bind/r", 16, q)
    for log2n in (1, 2, 3, 4, NLOG):
        h = 1 << (log2n - 1)
        for var in range(log2n):
            r = (0, 1, q - 1)[var] if log2n == 4 and var < 3 else rs[var]       # the shortcut-looking scalars are ordinary input
            for m in (1, 8):
                ctx.scalars_bind(dsts[:m], ptrs[:m], log2n, var, r)
                for j in range(m):
                    assert f.read(dsts[j], h) == bind_ref(vals[j], log2n, var, r, q), (f.name, log2n, var, m, j)
    for j in range(8):
        assert f.read(ptrs[j], N) == vals[j] and f.is_sentinel(dsts[j] - 32) and f.is_sentinel(dsts[j] + 32 * (N // 2))


def test_bind_in_place_and_out_of_place(f7):
    f, q, ctx = f7, f7.q, f7.ctx
    h = N // 2
    V = [mixed(f.cv, f"inplace/{j}", N) for j in range(2)]
    r = _ints(f"{f.name}/inplace/r", 1, q)[0]
    v = [f.vector(x) for x in V]
    ctx.scalars_bind(v, v, NLOG, NLOG - 1, r)                                   # the top variable, in place, two tables at once
    for j in range(2):
        assert f.read(v[j], h) == bind_ref(V[j], NLOG, NLOG - 1, r, q)
        assert f.read(v[j] + 32 * h, h) == V[j][h:]                             # the upper half keeps its bytes
        assert f.is_sentinel(v[j] - 32) and f.is_sentinel(v[j] + 32 * N)
    # out of place into a buffer of n rows: the rows from h on are not touched
    src, dst = f.vector(V[0]), f.vector(N)
    for var in (0, NLOG - 1):
        ctx.scalars_bind(dst, src, NLOG, var, r)
        assert f.read(dst, h) == bind_ref(V[0], NLOG, var, r, q)
        assert ctx.device_download(dst + 32 * h, 32 * h) == SENTINEL * h
        assert f.is_sentinel(dst - 32) and f.read(src, N) == V[0]


# ---------------------------------------------------------------------------------------------- 3: eq

def test_eq_tables(f7):
    f, q, ctx = f7, f7.q, f7.ctx
    point = _ints(f"{f.name}/eq/r", 12, q)
    s = _ints(f"{f.name}/eq/s", 1, q)[0]
    d, scratch = f.vector(1 << 12), f.vector(1 << 12)
    for v in range(13):
        n = 1 << v
        for scale in (None, s):
            ctx.device_upload(d, SENTINEL * n)
            ctx.scalars_eq(d, point[:v], scale)
            assert f.read(d, n) == eq_ref(point[:v], 1 if scale is None else scale, q), (f.name, v, scale)
            assert f.last()[3] == (v + 1) // 2
            assert f.is_sentinel(d - 32) and (v == 12 or f.is_sentinel(d + 32 * n))
            # the table sums to its scale
            assert ctx.scalars_scan(scratch, d, n) == (1 if scale is None else scale)
    assert f.is_sentinel(d + 32 * (1 << 12))
    # a point of zeros and ones gives the indicator vector of its index, times the scale
    bits = [(5 * j + 1) % 3 % 2 for j in range(11)]
    idx = sum(b << j for j, b in enumerate(bits))
    ctx.scalars_eq(d, bits, q - 1)
    assert f.read(d, 1 << 11) == [(q - 1) * int(i == idx) for i in range(1 << 11)]
    ctx.scalars_eq(d, [q - 1, 0, 1], 0)
    assert f.read(d, 8) == [0] * 8
    # f(r) = <eq(r), f> is the table bound variable by variable
    vals, ptrs = f.tables()
    ctx.scalars_eq(d, point[:NLOG])
    cur = vals[0]
    for j in range(NLOG):
        cur = bind_ref(cur, NLOG - j, 0, point[j], q)
    assert ctx.scalars_inner(d, ptrs[0], N) == cur[0]


# ---------------------------------------------------------------------------------------------- 4: whole protocols

@pytest.mark.parametrize("order", ["top_in_place", "var0_out_of_place"])
@pytest.mark.parametrize("case", ["prod2", "eq_prod3", "r1cs"])
def test_a_whole_sumcheck(f7, case, order):
    """v = 10 rounds of round -> challenge -> bind.  Per round s(0) + s(1) is the running claim and the next claim is s(r).
    At the end every table has shrunk to one scalar, which is <eq(point), original table>, and g of those is the last claim."""
    f, q, ctx = f7, f7.q, f7.ctx
    vals, orig = f.tables()
    tau = _ints(f"{f.name}/proto/tau", NLOG, q)
    shape, m = {"prod2": ("prod", 2), "eq_prod3": ("prod", 3), "r1cs": ("r1cs", 4)}[case]
    tables = [list(v) for v in vals[:m]]
    if case != "prod2":
        tables[0] = eq_ref(tau, 1, q)                                           # f_0 = eq(tau, .)
    # working copies, which the binds overwrite; the originals stay for the final check
    work = [f.vector(t) for t in tables]
    if case != "prod2":
        ctx.scalars_eq(work[0], tau)
        assert f.read(work[0], N) == tables[0]
        first = f.vector(N)
        ctx.scalars_eq(first, tau)
        firsts = [first] + orig[1:m]
    else:
        firsts = orig[:m]
    spare = [f.vector(N // 2) for _ in range(m)]
    claim = sum(g_of(shape, [t[i] for t in tables], q) for i in range(N)) % q
    if case == "prod2":
        assert ctx.scalars_inner(work[0], work[1], N) == claim
    challenges = _ints(f"{f.name}/proto/{case}/{order}", NLOG, q)
    point = [None] * NLOG
    cur = work
    for k, r in enumerate(challenges):
        log2n = NLOG - k
        var = log2n - 1 if order == "top_in_place" else 0
        evals = ctx.scalars_sumcheck_round(cur, log2n, var, shape)
        assert len(evals) == degree(shape, m) + 1
        assert (evals[0] + evals[1]) % q == claim, (f.name, case, order, k)
        claim = interpolate(evals, r, q)
        if order == "top_in_place":
            ctx.scalars_bind(cur, cur, log2n, var, r)
            point[NLOG - 1 - k] = r                                             # the top variable of what is left
        else:
            nxt = spare if cur is work else work
            ctx.scalars_bind(nxt, cur, log2n, var, r)
            cur = nxt
            point[k] = r                                                        # variable 0 of what is left is variable k of the table
    finals = [f.read(p, 1)[0] for p in cur]
    eq_pt = f.vector(N)
    ctx.scalars_eq(eq_pt, point)
    for j in range(m):
        assert finals[j] == ctx.scalars_inner(eq_pt, firsts[j], N), (f.name, case, order, j)
        assert finals[j] == sum(e * t for e, t in zip(eq_ref(point, 1, q), tables[j])) % q
    assert g_of(shape, finals, q) == claim


# ---------------------------------------------------------------------------------------------- 5: refusals

def test_every_refusal_leaves_outputs_and_context_as_they_were(f7):
    from montgomery_amd._lib import MSM_ERR_ARG, MSM_ERR_SCALAR, SUMCHECK_PROD, SUMCHECK_R1CS

    f, q, ctx = f7, f7.q, f7.ctx
    lib, h = ctx._lib, ctx._h
    vals, ptrs = f.tables()
    log2n, half = 6, 32
    W = mixed(f.cv, "bad/w", 64)
    w, w2, d, d2 = f.vector(W), f.vector(W), f.vector(64), f.vector(64)
    r_ok = _ints(f"{f.name}/bad/r", 1, q)[0]
    good_round = round_ref(vals[:2], log2n, 2, "prod", q)
    good_bind = bind_ref(W, log2n, 2, r_ok, q)
    vp = ctypes.c_void_p

    def arr(*p):
        return (vp * 8)(*[None if x is None else vp(x) for x in p])

    def buf(v):
        return (ctypes.c_uint8 * 32).from_buffer_copy(v.to_bytes(32, "little"))

    def still_good():
        assert f.read(w, 64) == W and f.read(w2, 64) == W and ctx.device_download(d, 64 * 32) == SENTINEL * 64
        assert ctx.device_download(d2, 64 * 32) == SENTINEL * 64
        assert ctx.scalars_sumcheck_round(ptrs[:2], log2n, 2) == good_round
        ctx.scalars_bind(d, w, log2n, 2, r_ok)
        assert f.read(d, half) == good_bind and ctx.device_download(d + 32 * half, 32 * half) == SENTINEL * half
        ctx.device_upload(d, SENTINEL * 64)

    def round_refused(code, vecs, m, lg, var, shape):
        out = (ctypes.c_uint8 * 160)(*([7] * 160))
        assert lib.msm_scalars_sumcheck_round(h, vecs, m, lg, var, shape, out) == code, (m, lg, var, shape)
        assert bytes(out) == bytes([7] * 160) and f.last()[:3] == [0, 0, 0]
        still_good()

    def bind_refused(code, dst, a, m, lg, var, r=r_ok):
        assert lib.msm_scalars_bind(h, dst, a, m, lg, var, None if r is None else buf(r)) == code, (m, lg, var)
        still_good()

    def eq_refused(code, dst, r_vals, v, s):
        rb = (ctypes.c_uint8 * (32 * max(len(r_vals), 1))).from_buffer_copy(to_bytes(r_vals) or bytes(32))
        assert lib.msm_scalars_eq(h, None if dst is None else vp(dst), rb, v, None if s is None else buf(s)) == code, (v, s)
        assert f.last()[3] == -1
        still_good()

    four = arr(*ptrs[:4])
    # the round: m, log2n, var, shape
    round_refused(MSM_ERR_ARG, four, 0, log2n, 0, SUMCHECK_PROD)
    round_refused(MSM_ERR_ARG, arr(*ptrs[:5]), 5, log2n, 0, SUMCHECK_PROD)
    for m in (1, 2, 3, 5):
        round_refused(MSM_ERR_ARG, arr(*ptrs[:5]), m, log2n, 0, SUMCHECK_R1CS)
    round_refused(MSM_ERR_ARG, four, 2, 0, 0, SUMCHECK_PROD)
    round_refused(MSM_ERR_ARG, four, 2, 30, 0, SUMCHECK_PROD)
    round_refused(MSM_ERR_ARG, four, 2, log2n, log2n, SUMCHECK_PROD)
    round_refused(MSM_ERR_ARG, four, 2, log2n, 0, 2)
    round_refused(MSM_ERR_ARG, four, 2, log2n, 0, -1)
    # null and misaligned vectors, a null array, a null output
    round_refused(MSM_ERR_ARG, arr(ptrs[0], None), 2, log2n, 0, SUMCHECK_PROD)
    round_refused(MSM_ERR_ARG, arr(ptrs[0], ptrs[1], ptrs[2], ptrs[3] + 8), 4, log2n, 0, SUMCHECK_R1CS)
    round_refused(MSM_ERR_ARG, arr(ptrs[0] + 4), 1, log2n, 0, SUMCHECK_PROD)
    round_refused(MSM_ERR_ARG, None, 2, log2n, 0, SUMCHECK_PROD)
    assert lib.msm_scalars_sumcheck_round(h, four, 2, log2n, 0, SUMCHECK_PROD, None) == MSM_ERR_ARG
    still_good()
    # bind: the same ranges, then the scalar
    bind_refused(MSM_ERR_ARG, arr(d), arr(w), 0, log2n, 0)
    bind_refused(MSM_ERR_ARG, arr(*[d] * 8), arr(*[w] * 8), 9, log2n, 0)
    bind_refused(MSM_ERR_ARG, arr(d), arr(w), 1, 0, 0)
    bind_refused(MSM_ERR_ARG, arr(d), arr(w), 1, 30, 0)
    bind_refused(MSM_ERR_ARG, arr(d), arr(w), 1, log2n, log2n)
    bind_refused(MSM_ERR_ARG, arr(None), arr(w), 1, log2n, 0)
    bind_refused(MSM_ERR_ARG, arr(d, d2), arr(w, None), 2, log2n, 0)
    bind_refused(MSM_ERR_ARG, arr(d + 8), arr(w), 1, log2n, 0)
    bind_refused(MSM_ERR_ARG, arr(d), arr(w + 8), 1, log2n, 0)
    bind_refused(MSM_ERR_ARG, None, arr(w), 1, log2n, 0)
    bind_refused(MSM_ERR_ARG, arr(d), None, 1, log2n, 0)
    bind_refused(MSM_ERR_ARG, arr(d), arr(w), 1, log2n, 0, None)
    bind_refused(MSM_ERR_SCALAR, arr(d), arr(w), 1, log2n, 0, q)
    bind_refused(MSM_ERR_SCALAR, arr(d), arr(w), 1, log2n, 0, TOP)
    # every forbidden overlap: in place below the top variable; a destination inside its source, at either end of it and
    # across its end; inside another source; on another destination, wholly and in part; in place on another table's source
    top = log2n - 1
    bind_refused(MSM_ERR_ARG, arr(w), arr(w), 1, log2n, top - 1)
    bind_refused(MSM_ERR_ARG, arr(w), arr(w), 1, log2n, 0)
    bind_refused(MSM_ERR_ARG, arr(w + 32), arr(w), 1, log2n, top)
    bind_refused(MSM_ERR_ARG, arr(w + 32 * half), arr(w), 1, log2n, top)
    bind_refused(MSM_ERR_ARG, arr(w + 32 * 63), arr(w), 1, log2n, top)
    bind_refused(MSM_ERR_ARG, arr(w - 32 * (half - 1)), arr(w), 1, log2n, top)
    bind_refused(MSM_ERR_ARG, arr(d, w2 + 32 * 8), arr(w, w2), 2, log2n, top)
    bind_refused(MSM_ERR_ARG, arr(d, w), arr(w, w2), 2, log2n, top)
    bind_refused(MSM_ERR_ARG, arr(d, d), arr(w, w2), 2, log2n, top)
    bind_refused(MSM_ERR_ARG, arr(d, d + 32 * (half - 1)), arr(w, w2), 2, log2n, top)
    bind_refused(MSM_ERR_ARG, arr(w, d), arr(w, w), 2, log2n, top)
    # eq: v, the pointers, the scalars
    point = _ints(f"{f.name}/bad/eq", 4, q)
    eq_refused(MSM_ERR_ARG, d, point, 30, None)
    eq_refused(MSM_ERR_ARG, None, point, 4, None)
    eq_refused(MSM_ERR_ARG, d + 8, point, 4, None)
    eq_refused(MSM_ERR_SCALAR, d, point[:3] + [q], 4, None)
    eq_refused(MSM_ERR_SCALAR, d, [TOP] + point[1:], 4, 1)
    eq_refused(MSM_ERR_SCALAR, d, point, 4, q)
    assert lib.msm_scalars_eq(h, vp(d), None, 4, None) == MSM_ERR_ARG
    still_good()
    # and the valid neighbours of what was refused
    ctx.scalars_eq(d, point)
    assert f.read(d, 16) == eq_ref(point, 1, q) and f.last()[3] == 2
    ctx.device_upload(d, SENTINEL * 16)
    ctx.scalars_bind([w, d], [w, w2], log2n, top, r_ok)
    assert f.read(w, half) == bind_ref(W, log2n, top, r_ok, q) == f.read(d, half) and f.read(w + 32 * half, half) == W[half:]


def test_device_list_contexts_are_refused():
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError
    from montgomery_amd.api import MsmContext

    multi = MsmContext(D.CURVE_TABLE["bls377"].cid, devices=[0, 0])
    try:
        p, d = multi.device_alloc(128), multi.device_alloc(128)
        multi.device_upload(p, bytes(128))
        multi.device_upload(d, bytes(128))
        for call in (lambda: multi.scalars_sumcheck_round([p, p], 2, 0), lambda: multi.scalars_bind(d, p, 2, 1, 3),
                     lambda: multi.scalars_eq(d, [2, 3])):
            with pytest.raises(MsmError) as e:
                call()
            assert e.value.code == MSM_ERR_ARG
        assert multi._lib.msm_test_set_sumcheck_grid(multi._h, 1) == MSM_ERR_ARG
        assert multi._lib.msm_test_last_sumcheck(multi._h, (ctypes.c_int32 * 4)(), 4) == -1
        assert multi.device_download(p, 128) == bytes(128) and multi.device_download(d, 128) == bytes(128)
    finally:
        multi.close()
