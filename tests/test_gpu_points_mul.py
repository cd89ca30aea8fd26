"""msm_points_mul / msm_points_mul_base: D[i] = s[i] * A[a_lo + i] and D[i] = s[i] * P on the GPU.  `-m gpu`.

The fixture is that of tests/test_gpu_points_lincomb.py: sets of 336 generated points with known logs (P_i = k_i G) on all seven
curves, so a produced row has the expected value (s_i k_i mod q) G from the oracle; degenerate rows come from the pool of
tests/degenerate_inputs.py and are expected through cv.scale.  Counts are 1, 64, 65 and 321."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degenerate_inputs as D  # noqa: E402
import digit_model as M  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402
from test_gpu_points_lincomb import COUNTS, N7, Fix  # noqa: E402

pytestmark = pytest.mark.gpu
TWO256 = 1 << 256
PATH_VAR, PATH_TABLE, PATH_BROADCAST = 0, 1, 2


def _ints(tag, n, bound):
    return O.prng_ints(f"points_mul/{tag}", n, bound)


def sbytes(scalars):
    return b"".join(int(s).to_bytes(32, "little") for s in scalars)


def last_call(ctx):
    """(grid, w, path, table rows) of the last msm_points_mul / msm_points_mul_base, from the library's own report"""
    out = (ctypes.c_int32 * 4)()
    assert ctx._lib.msm_test_last_points_mul(ctx._h, out, 4) == 4
    return tuple(out)


def set_grid(ctx, blocks):
    ctx._check(ctx._lib.msm_test_set_points_mul_grid(ctx._h, blocks))


def set_base_path(ctx, path):
    ctx._check(ctx._lib.msm_test_set_points_mul_base_path(ctx._h, path))


def edge_scalars(cv):
    """the list of tests/test_points_mul_host.py"""
    q = cv.q
    out = [0, 1, 2, q - 2, q - 1, q, q + 1, TWO256 - 1]
    if not cv.te:
        out += [cv.B.lam, q - cv.B.lam]
    low, high = M.fixed_scalars(cv)
    return list(dict.fromkeys(out + low + high))


@pytest.fixture(scope="module", params=D.NAMES)
def f7(request):
    f = Fix(request.param)
    yield f
    f.ctx.close()


@pytest.fixture(scope="module")
def f377():
    f = Fix("bls377")
    yield f
    f.ctx.close()


# ---------------------------------------------------------------------------------------------- 1: generic

def test_generic_rows_and_msm_over_the_result(f7):
    f, cv, q, ctx = f7, f7.cv, f7.q, f7.ctx
    a_lo, n = 3, COUNTS[-1]
    s = _ints(f"{f.name}/s", n, q)
    assert ctx.points_mul(sbytes(s), src=f.sa, a_lo=a_lo, dst=f.sd) == n
    grid, w, path, t_rows = last_call(ctx)
    assert grid == 2 and path == PATH_VAR and t_rows == 0 and w in (3, 4, 5)
    assert ctx.pointset_size(f.sd) == n and ctx._cur_set == f.sa and ctx.pointset_size() == N7
    dlog = [(s[i] * f.la[a_lo + i]) % q for i in range(n)]
    wire = f.rows(f.sd, 0, n)
    assert wire == cv.wire([cv.scale_g(k) for k in dlog])
    # an MSM over the produced rows, with the endomorphism (it reads the beta x line) and without
    t = _ints(f"{f.name}/t", n, q)
    exp = cv.scale_g(sum(u * k for u, k in zip(t, dlog)) % q)
    glv, _ = f.run_on(f.sd, t)
    plain, _ = f.run_on(f.sd, t, no_glv=True)
    assert f.point(glv) == exp and f.point(plain) == exp
    # scalars from the device give the same bytes
    dev = ctx.device_alloc(32 * n)
    try:
        ctx.device_upload(dev, sbytes(s))
        assert ctx.points_mul(dev, src=f.sa, a_lo=a_lo, count=n, dst=f.sd) == n
        assert f.rows(f.sd, 0, n) == wire
    finally:
        ctx.device_free(dev)
    # the smaller counts write the same leading rows and leave exactly `count` of them
    for count in COUNTS[:-1]:
        assert ctx.points_mul(sbytes(s), src=f.sa, a_lo=a_lo, count=count, dst=f.sd) == count
        assert ctx.pointset_size(f.sd) == count
        assert f.rows(f.sd, 0, count) == wire[:f.step * count], (f.name, count)
    assert ctx.points_mul(b"", src=f.sa, dst=f.sd) == 0 and ctx.pointset_size(f.sd) == 0


# ---------------------------------------------------------------------------------------------- 2: grid-stride and slot reuse

def test_one_block_takes_two_rows_per_lane(f7):
    f, cv, q, ctx = f7, f7.cv, f7.q, f7.ctx
    n = COUNTS[-1]
    s = _ints(f"{f.name}/grid", n, q)
    ctx.points_mul(sbytes(s), src=f.sa, a_lo=3, dst=f.sd)
    assert last_call(ctx)[0] == 2
    want = f.rows(f.sd, 0, n)
    set_grid(ctx, 1)
    try:
        ctx.points_mul(sbytes(s), src=f.sa, a_lo=3, dst=f.sd)
        assert last_call(ctx)[0] == 1                      # 321 rows, 256 lanes: lanes 0 .. 64 take two rows over the same slots
        assert f.rows(f.sd, 0, n) == want
    finally:
        set_grid(ctx, 0)
    assert want == cv.wire([cv.scale_g(s[i] * f.la[3 + i] % q) for i in range(n)])


# ---------------------------------------------------------------------------------------------- 3: edge scalars in one wave

def test_edge_scalars_beside_ordinary_ones(f7):
    f, cv, q, ctx = f7, f7.cv, f7.q, f7.ctx
    edges = edge_scalars(cv)
    rnd = _ints(f"{f.name}/edge", len(edges), q)
    s = [v for pair in zip(edges, rnd) for v in pair]          # edge, ordinary, edge, ordinary ...
    n = len(s)
    assert n <= N7
    ctx.points_mul(sbytes(s), src=f.sa, dst=f.sd)
    exp = [cv.scale_g((v % q) * f.la[i] % q) for i, v in enumerate(s)]
    assert f.rows(f.sd, 0, n) == cv.wire(exp)
    assert exp[0] == cv.zero and f.points(f.sd, 2, 1) == f.points(f.sa, 2, 1)          # the scalars 0 and 1
    assert f.points(f.sd, 8, 1) == [cv.neg(f.points(f.sa, 8, 1)[0])]                    # q - 1: the negative
    # the same scalars on one base
    ctx.points_mul_base(sbytes(s), dst=f.sd)
    assert f.rows(f.sd, 0, n) == cv.wire([cv.scale_g(v % q) for v in s])


# ---------------------------------------------------------------------------------------------- 4: degenerate rows in one wave

def test_degenerate_rows_beside_ordinary_ones(f7):
    f, cv, q, ctx, n = f7, f7.cv, f7.q, f7.ctx, 128
    pts = D.pool(cv.name)[0]
    Z = cv.zero
    rows = []
    for i in range(n):
        P = pts[i % 5]
        rows.append({0: P, 1: Z, 2: P, 3: cv.neg(P), 4: pts[5 + i % 7], 5: P, 6: Z, 7: cv.neg(pts[i % 3])}[i % 8])
    s = _ints(f"{f.name}/deg", n, q)
    s[0:8] = [s[0]] * 8                                        # repeated and negated points under one scalar
    s[17], s[18], s[25] = 0, 1, q - 1
    src = ctx.pointset_create()
    try:
        ctx.pointset_select(src)
        ctx.set_points(cv.wire(rows), check_curve=True)
        ctx.points_mul(sbytes(s), src=src, dst=f.sd)
        exp = [Z if P == Z else cv.scale(v, P) for v, P in zip(s, rows)]
        assert f.rows(f.sd, 0, n) == cv.wire(exp), f.name
        ctx.pointset_select(f.sd)
        ctx.validate_points(0, n, "curve")
    finally:
        ctx.pointset_select(f.sa)
        ctx.pointset_destroy(src)


def torsion_rows(cv):
    """Points outside the prime-order subgroup.  BLS12-377: (p - 1, 0) of order 2 (tests/degenerate_inputs.py) and (0, 1) of order
    3.  BLS12-381: (0, 2) of order 3 -- its cofactor is odd, the curve has no point of even order; 3 T = O still puts the identity
    into the lane's table (Z = 0 under the shared inversion), which is the case an even order makes on BLS12-377."""
    if cv.name == "bls377":
        out = [D.torsion_points(cv)[0][0], (0, 1)]
    else:
        out = [(0, 2), (0, cv.p - 2)]
    for T in out:
        assert O.aff_is_on_curve(T, cv.B)
    return out


@pytest.mark.parametrize("name", ["bls377", "bls381"])
def test_a_torsion_row_leaves_its_neighbours_alone(name):
    """Torsion rows next to ordinary ones in one wave: the call returns and every other row is right.  What the torsion rows
    themselves become is outside the contract (the endomorphism is not lambda on them)."""
    from montgomery_amd.api import MsmContext

    cv = D.CURVE_TABLE[name]
    q, n = cv.q, 65
    ctx = MsmContext(cv.cid)
    try:
        pts = D.pool(name)[0]
        rows = [pts[i % D.POOL] for i in range(n)]
        tors = torsion_rows(cv)
        at = {5: tors[0], 6: tors[0], 40: tors[1], 64: tors[1]}
        for i, T in at.items():
            rows[i] = T
        s = _ints(f"{name}/torsion", n, q)
        ctx.set_points(cv.wire(rows), check_curve=True)
        dst = ctx.pointset_create()
        assert ctx.points_mul(sbytes(s), src=0, dst=dst) == n
        assert ctx.pointset_size(dst) == n
        got = ctx.get_points(0, n)
        step = 2 * ctx.coord_bytes
        for i in range(n):
            if i not in at:
                assert got[step * i:step * (i + 1)] == cv.wire([cv.scale(s[i], rows[i])]), (name, i)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 5: in place

@pytest.mark.parametrize("name", ["bls377", "ed377"])
def test_in_place(name):
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError
    from montgomery_amd.api import MsmContext

    cv = D.CURVE_TABLE[name]
    q, n = cv.q, 642
    ctx = MsmContext(cv.cid)
    try:
        logs = O.scalars_from_bytes(ctx.generate_points(n, seed=1503, want_scalars=True))
        s = _ints(f"{name}/inplace", n // 2, q)
        before = ctx.get_points(0, n)
        for a_lo in (1, n // 2 - 1):                           # a source range that overlaps the rows written
            with pytest.raises(MsmError) as e:
                ctx.points_mul(sbytes(s), a_lo=a_lo)
            assert e.value.code == MSM_ERR_ARG
        assert ctx.pointset_size() == n and ctx.get_points(0, n) == before
        # a_lo = count: the upper half under s lands in the lower half, the set is truncated
        assert ctx.points_mul(sbytes(s), a_lo=n // 2) == n // 2
        assert ctx.pointset_size() == n // 2 == ctx.n_points
        assert ctx.get_points(0, n // 2) == cv.wire([cv.scale_g(s[i] * logs[n // 2 + i] % q) for i in range(n // 2)])
        with pytest.raises(MsmError):
            ctx.get_points(n // 2, 1)
        # a_lo = 0: row i under t[i], on top of the rows just written
        t = _ints(f"{name}/inplace2", 65, q)
        assert ctx.points_mul(sbytes(t)) == 65 and ctx.pointset_size() == 65
        assert ctx.get_points(0, 65) == cv.wire([cv.scale_g(t[i] * s[i] * logs[n // 2 + i] % q) for i in range(65)])
    finally:
        ctx.close()


def test_in_place_drops_the_tables_of_its_set_only(f377):
    f, ctx, q, n = f377, f377.ctx, f377.q, 4096
    kept, work = ctx.pointset_create(), None
    try:
        ctx.generate_points(n, seed=1504)
        assert ctx.precompute()[1] >= 2
        kept_tables = ctx.tables_info()
        work = ctx.pointset_create()
        logs = O.scalars_from_bytes(ctx.generate_points(n, seed=1505, want_scalars=True))
        assert ctx.precompute()[1] >= 2
        s = _ints("tables/s", 321, q)
        assert ctx.points_mul(sbytes(s)) == 321
        assert ctx._cur_set == work and ctx.tables_info() == (0, 0, 0) and ctx.pointset_size() == 321
        t = _ints("tables/t", 321, q)
        got, info = ctx.run(O.scalars_to_bytes(t))
        assert not info["tables"]
        assert f.point(got) == f.cv.scale_g(sum(u * v * k for u, v, k in zip(t, s, logs)) % q)
        # from another set: the set that is read keeps its tables
        ctx.pointset_select(kept)
        ctx.points_mul(sbytes(s), src=kept, dst=work)
        assert ctx._cur_set == kept and ctx.tables_info() == kept_tables and ctx.pointset_size() == n
        # window tables on a produced set, and a linear combination of it
        ctx.points_mul_base(sbytes(_ints("tables/base", n, q)), dst=work)
        ctx.pointset_select(work)
        assert ctx.precompute()[1] >= 2
        u = _ints("tables/u", n, q)
        on_tables, info = ctx.run(O.scalars_to_bytes(u))
        plain, _ = ctx.run(O.scalars_to_bytes(u), no_tables=True)
        assert info["tables"] and on_tables == plain
        assert f.point(plain) == f.cv.scale_g(sum(a * b for a, b in zip(u, _ints("tables/base", n, q))) % q)
        ctx.points_lincomb(3, src_a=work, count=8, dst=work)
        assert f.rows(work, 0, 8) == f.cv.wire([f.cv.scale_g(3 * b % q) for b in _ints("tables/base", 8, q)])
    finally:
        ctx.pointset_select(f.sa)
        ctx.pointset_destroy(kept)
        if work is not None:
            ctx.pointset_destroy(work)


# ---------------------------------------------------------------------------------------------- 6: fixed base

def test_fixed_base_both_paths_and_the_cache(f7):
    f, cv, q, ctx = f7, f7.cv, f7.q, f7.ctx
    n = COUNTS[-1]
    s = _ints(f"{f.name}/base", n, q)
    P1, P2 = f.points(f.sa, 5, 1)[0], f.points(f.sb, 9, 1)[0]
    k1, k2 = f.la[5], f.lb[9]
    try:
        # G (NULL) on both paths: the same bytes, the expected rows
        set_base_path(ctx, PATH_BROADCAST)
        assert ctx.points_mul_base(sbytes(s), dst=f.sd) == n
        grid, w, path, t_rows = last_call(ctx)
        assert path == PATH_BROADCAST and t_rows == 0 and grid == 2
        wire_g = f.rows(f.sd, 0, n)
        assert wire_g == cv.wire([cv.scale_g(v) for v in s])
        set_base_path(ctx, PATH_TABLE)
        ctx.points_mul_base(sbytes(s), dst=f.sd)
        grid, wb, path, t_rows = last_call(ctx)
        assert path == PATH_TABLE and wb in (6, 8, 10) and grid == 2
        assert t_rows == -(-(cv.scalar_bits + 1) // wb) << (wb - 1)
        assert f.rows(f.sd, 0, n) == wire_g
        for count in COUNTS[:-1]:
            assert ctx.points_mul_base(sbytes(s), count=count, dst=f.sd) == count
            assert f.rows(f.sd, 0, count) == wire_g[:f.step * count]
        # P1, then P2, then P1 again on the table path: the cache never serves the table of another base
        w1 = cv.wire([cv.scale_g(v * k1 % q) for v in s[:65]])
        w2 = cv.wire([cv.scale_g(v * k2 % q) for v in s[:65]])
        for base, want in ((P1, w1), (P2, w2), (P1, w1), (None, wire_g[:f.step * 65]), (P1, w1)):
            ctx.points_mul_base(sbytes(s[:65]), None if base is None else cv.wire([base]), dst=f.sd)
            assert last_call(ctx)[2] == PATH_TABLE
            assert f.rows(f.sd, 0, 65) == want
        # automatic: the cached base takes its table, another base at this size the broadcast row
        set_base_path(ctx, 0)
        ctx.points_mul_base(sbytes(s[:65]), cv.wire([P1]), dst=f.sd)
        assert last_call(ctx)[2] == PATH_TABLE and f.rows(f.sd, 0, 65) == w1
        ctx.points_mul_base(sbytes(s[:65]), cv.wire([P2]), dst=f.sd)
        assert last_call(ctx)[2] == PATH_BROADCAST and f.rows(f.sd, 0, 65) == w2
        # the identity as a base, on both paths
        for path in (PATH_TABLE, PATH_BROADCAST):
            set_base_path(ctx, path)
            ctx.points_mul_base(sbytes(s[:65]), bytes(f.step) if not cv.te else cv.wire([cv.zero]), dst=f.sd)
            assert f.points(f.sd, 0, 65) == [cv.zero] * 65
        if cv.te:                                          # the all-zero encoding is the identity on the Edwards curve too
            ctx.points_mul_base(sbytes(s[:3]), bytes(f.step), dst=f.sd)
            assert f.points(f.sd, 0, 3) == [cv.zero] * 3
    finally:
        set_base_path(ctx, 0)


def test_kzg_commitment_without_a_host_side_srs(f7):
    """scalars_powers(tau) -> points_mul_base -> msm_run with coefficients c equals (sum c_i tau^i) G."""
    f, cv, q, ctx = f7, f7.cv, f7.q, f7.ctx
    n = COUNTS[-1]
    tau = _ints(f"{f.name}/tau", 1, q)[0] or 7
    dev = ctx.device_alloc(32 * n)
    try:
        set_base_path(ctx, PATH_TABLE)
        ctx.scalars_powers(dev, tau, n)
        assert ctx.points_mul_base(dev, count=n, dst=f.sd) == n
        assert last_call(ctx)[2] == PATH_TABLE
        assert f.points(f.sd, 0, 3) == [cv.scale_g(1), cv.scale_g(tau), cv.scale_g(tau * tau % q)]
        c = _ints(f"{f.name}/coeff", n, q)
        got, _ = f.run_on(f.sd, c)
        assert f.point(got) == cv.scale_g(sum(ci * pow(tau, i, q) for i, ci in enumerate(c)) % q)
    finally:
        set_base_path(ctx, 0)
        ctx.device_free(dev)


# ---------------------------------------------------------------------------------------------- 7: under a workspace limit

def test_a_workspace_limit_shrinks_the_grid(f7):
    f, cv, q, ctx = f7, f7.cv, f7.q, f7.ctx
    n = COUNTS[-1]
    s = _ints(f"{f.name}/limit", n, q)
    ctx.points_mul(sbytes(s), src=f.sa, a_lo=3, dst=f.sd)
    assert last_call(ctx)[0] == 2
    want = f.rows(f.sd, 0, n)
    per_block = 256 * (1 << (last_call(ctx)[1] - 1)) * 4 * ctx.coord_bytes      # lanes x entries x coordinates x bytes
    try:
        ctx.set_workspace_limit(per_block + per_block // 2)    # room for one block's tables, not for two
        ctx.points_mul(sbytes(s), src=f.sa, a_lo=3, dst=f.sd)
        assert last_call(ctx)[0] == 1
        assert f.rows(f.sd, 0, n) == want
        ctx.set_workspace_limit(1 << 12)                   # room for none: the grid stops at one block
        ctx.points_mul(sbytes(s), src=f.sa, a_lo=3, dst=f.sd)
        assert last_call(ctx)[0] == 1
        assert f.rows(f.sd, 0, n) == want
    finally:
        ctx.set_workspace_limit(0)


# ---------------------------------------------------------------------------------------------- errors on a live context

def test_every_refusal_leaves_the_sets_as_they_were(f7):
    from montgomery_amd._lib import MSM_ERR_ARG, MSM_ERR_NO_POINTS, MSM_ERR_POINT, MSM_OK, MsmError
    from montgomery_amd.api import MsmContext

    f, cv, q, ctx = f7, f7.cv, f7.q, f7.ctx
    lib, h = ctx._lib, ctx._h
    s = _ints(f"{f.name}/err", 65, q)
    ctx.points_mul(sbytes(s), src=f.sa, dst=f.sd)
    before = f.rows(f.sd, 0, 65)
    src_before = f.rows(f.sa, 0, N7)

    def still_good():
        assert ctx.pointset_size(f.sd) == 65 and f.rows(f.sd, 0, 65) == before
        assert ctx.pointset_size(f.sa) == N7 and f.rows(f.sa, 0, N7) == src_before

    dead = ctx.pointset_create()
    ctx.pointset_destroy(dead)
    ctx.pointset_select(f.sa)
    buf = (ctypes.c_uint8 * (32 * 65)).from_buffer_copy(sbytes(s))
    dev = ctx.device_alloc(32 * 66)
    try:
        bad = [
            (MSM_ERR_ARG, (99, 0, buf, 0, 1, f.sd)), (MSM_ERR_ARG, (f.sa, 0, buf, 0, 1, 99)), (MSM_ERR_ARG, (dead, 0, buf, 0, 1, f.sd)),
            (MSM_ERR_ARG, (f.sa, 0, buf, 0, 1, -1)), (MSM_ERR_ARG, (f.sa, 0, None, 0, 1, f.sd)),
            (MSM_ERR_ARG, (f.sa, 0, ctypes.c_void_p(dev + 8), 1, 1, f.sd)), (MSM_ERR_ARG, (f.sa, 0, buf, 0, 1 << 30, f.sd)),
            (MSM_ERR_ARG, (f.sd, 1, buf, 0, 8, f.sd)),
            (MSM_ERR_NO_POINTS, (f.sa, N7 - 3, buf, 0, 4, f.sd)),
        ]
        for code, args in bad:
            assert lib.msm_points_mul(h, *args) == code, args
            still_good()
        for code, args in ((MSM_ERR_ARG, (None, buf, 0, 1, 99)), (MSM_ERR_ARG, (None, None, 0, 1, f.sd)),
                           (MSM_ERR_ARG, (None, ctypes.c_void_p(dev + 4), 1, 1, f.sd)), (MSM_ERR_ARG, (None, buf, 0, 1 << 30, f.sd))):
            assert lib.msm_points_mul_base(h, *args) == code, args
            still_good()
        # a base off the curve, and one with a coordinate >= p
        P = f.points(f.sa, 0, 1)[0]
        off = cv.wire([(P[0], (P[1] + 1) % cv.p)])
        big = cv.p.to_bytes(ctx.coord_bytes, "little") + P[1].to_bytes(ctx.coord_bytes, "little")
        for base in (off, big):
            with pytest.raises(MsmError) as e:
                ctx.points_mul_base(sbytes(s), base, dst=f.sd)
            assert e.value.code == MSM_ERR_POINT
            still_good()
        assert lib.msm_points_mul(h, f.sa, 0, None, 0, 0, f.sd) == MSM_OK      # count == 0 needs no scalars
        assert ctx.pointset_size(f.sd) == 0
    finally:
        ctx.device_free(dev)
    multi = MsmContext(cv.cid, devices=[0, 0])
    try:
        multi.generate_points(8, seed=3)
        for call in (lambda: multi.points_mul(sbytes(s[:8])), lambda: multi.points_mul_base(sbytes(s[:8]))):
            with pytest.raises(MsmError) as e:
                call()
            assert e.value.code == MSM_ERR_ARG
        assert len(multi.get_points(0, 8)) == 8 * f.step
    finally:
        multi.close()
