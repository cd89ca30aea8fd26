"""msm_points_lincomb: D[i] = a * A[a_lo + i] + b * B[b_lo + i] over resident rows, on the GPU.  `-m gpu`.

Generated point sets come with their discrete logs (P_i = k_i G), so a produced row has the expected value
((a alpha_i + b beta_i) mod q) G from the oracle; degenerate lanes are built from wire points of the pool of
tests/degenerate_inputs.py and expected through cv.add / cv.scale.  Sizes are the smallest that cross a wave (64) and a block
(256) with a ragged tail: 1, 64, 65, 321."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degenerate_inputs as D  # noqa: E402
from operator_fixture import OperatorFixture  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

N7 = 336          # points of the two generated sets of the all-curves fixture: 321 rows from row 3 / row 7 on
COUNTS = (1, 64, 65, 321)


def _ints(tag, n, bound):
    return O.prng_ints(f"lincomb/{tag}", n, bound)


class Fix(OperatorFixture):
    """One context per curve with two generated sets A (the default set) and B with known logs, and an empty third set."""

    def __init__(self, name):
        super().__init__(name)
        self.sa = 0
        self.la = O.scalars_from_bytes(self.ctx.generate_points(N7, seed=1401, want_scalars=True))
        self.sb = self.ctx.pointset_create()
        self.lb = O.scalars_from_bytes(self.ctx.generate_points(N7, seed=1402, want_scalars=True))
        self.sd = self.ctx.pointset_create()
        self.ctx.pointset_select(self.sa)
        self.step = 2 * self.ctx.coord_bytes

    def rows(self, set_id, first, count):
        """wire bytes of rows [first, first + count) of a set; the current set is put back"""
        cur = self.ctx._cur_set
        self.ctx.pointset_select(set_id)
        try:
            return self.ctx.get_points(first, count)
        finally:
            self.ctx.pointset_select(cur)

    def points(self, set_id, first, count):
        """the same as affine points in the form Curve.scale_g gives"""
        raw, cb = self.rows(set_id, first, count), self.ctx.coord_bytes
        out = []
        for i in range(count):
            x = int.from_bytes(raw[self.step * i:self.step * i + cb], "little")
            y = int.from_bytes(raw[self.step * i + cb:self.step * (i + 1)], "little")
            out.append(None if (x, y) == (0, 0) else (x, y))
        return out

    def run_on(self, set_id, scalars, **kw):
        cur = self.ctx._cur_set
        self.ctx.pointset_select(set_id)
        try:
            return self.ctx.run(O.scalars_to_bytes(scalars), **kw)
        finally:
            self.ctx.pointset_select(cur)

    def add(self, P, Q):
        cv = self.cv
        if not cv.te:
            if P is None:
                return Q
            if Q is None:
                return P
        return cv.add(P, Q)


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
    a, b = [v or 1 for v in _ints(f"{f.name}/ab", 2, q)]
    a_lo, b_lo, n = 3, 7, COUNTS[-1]
    assert ctx.points_lincomb(a, b, src_a=f.sa, a_lo=a_lo, src_b=f.sb, b_lo=b_lo, count=n, dst=f.sd) == n
    assert ctx.pointset_size(f.sd) == n and ctx._cur_set == f.sa and ctx.pointset_size() == N7
    dlog = [(a * f.la[a_lo + i] + b * f.lb[b_lo + i]) % q for i in range(n)]
    wire = f.rows(f.sd, 0, n)
    assert wire == cv.wire([cv.scale_g(k) for k in dlog])
    # an MSM over the produced rows, with the endomorphism (it reads the beta x line) and without
    t = _ints(f"{f.name}/t", n, q)
    exp = cv.scale_g(sum(s * k for s, k in zip(t, dlog)) % q)
    glv, _ = f.run_on(f.sd, t)
    plain, _ = f.run_on(f.sd, t, no_glv=True)
    assert f.point(glv) == exp and f.point(plain) == exp
    # the smaller launches write the same rows (row i does not depend on count) and leave exactly `count` of them
    for count in COUNTS[:-1]:
        ctx.points_lincomb(a, b, src_a=f.sa, a_lo=a_lo, src_b=f.sb, b_lo=b_lo, count=count, dst=f.sd)
        assert ctx.pointset_size(f.sd) == count
        assert f.rows(f.sd, 0, count) == wire[:f.step * count], (f.name, count)
        tt = t[:count]
        got, _ = f.run_on(f.sd, tt)
        assert f.point(got) == cv.scale_g(sum(s * k for s, k in zip(tt, dlog)) % q)


# ---------------------------------------------------------------------------------------------- 2: shortcuts

def test_shortcut_scalars(f7):
    f, cv, q, ctx, n = f7, f7.cv, f7.q, f7.ctx, 65
    A, B = f.points(f.sa, 0, n), f.points(f.sb, 0, n)
    bb = _ints(f"{f.name}/b", 1, q)[0] or 5
    neg = cv.neg

    def dbl(P):
        return f.add(P, P)

    cases = [
        ((1, None), A),
        ((0, 0), [cv.zero] * n),
        ((q - 1, None), [neg(P) for P in A]),
        ((1, 1), [f.add(P, Q) for P, Q in zip(A, B)]),
        ((1, q - 1), [f.add(P, neg(Q)) for P, Q in zip(A, B)]),
        ((0, bb), None),
        ((2, None), [dbl(P) for P in A]),
        ((3, 1), [f.add(f.add(dbl(P), P), Q) for P, Q in zip(A, B)]),
    ]
    for (a, b), exp in cases:
        ctx.points_lincomb(a, b, src_a=f.sa, src_b=None if b is None else f.sb, count=n, dst=f.sd)
        assert ctx.pointset_size(f.sd) == n
        got = f.rows(f.sd, 0, n)
        if exp is not None:
            assert got == cv.wire(exp), (f.name, a, b)
        if (a, b) == (1, None):
            assert got == f.rows(f.sa, 0, n)               # the copy: the source's bytes
        t = _ints(f"{f.name}/t2", n, q)
        res, _ = f.run_on(f.sd, t)
        if (a, b) == (0, 0):
            assert f.point(res) == cv.zero
        if (a, b) == (0, bb):
            assert f.points(f.sd, 0, 3) == [cv.scale_g(bb * k) for k in f.lb[:3]]
            assert f.point(res) == cv.scale_g(sum(s * bb * k for s, k in zip(t, f.lb)) % q)


# ---------------------------------------------------------------------------------------------- 3: degenerate lanes in one wave

def _degenerate_pairs(cv, n):
    """n (A, B) pairs: generic lanes interleaved with identity rows, B = +-A, over six pool points"""
    pts = D.pool(cv.name)[0]
    Z = cv.zero
    out = []
    for i in range(n):
        P, Q = pts[i % 3], pts[3 + (i // 8) % 3]
        out.append({0: (P, Q), 1: (Z, Q), 2: (P, Z), 3: (Z, Z), 4: (P, P), 5: (P, cv.neg(P)), 6: (Q, P), 7: (Q, Q)}[i % 8])
    return out


def test_degenerate_lanes_next_to_generic_ones(f7):
    f, cv, q, ctx, n = f7, f7.cv, f7.q, f7.ctx, 128
    pairs = _degenerate_pairs(cv, n)
    sa, sb = ctx.pointset_create(), ctx.pointset_create()
    try:
        ctx.pointset_select(sa)
        ctx.set_points(cv.wire([p[0] for p in pairs]), check_curve=True)
        ctx.pointset_select(sb)
        ctx.set_points(cv.wire([p[1] for p in pairs]), check_curve=True)
        s = [v or 1 for v in _ints(f"{f.name}/deg", 2, q)]
        memo = {}

        def scale(k, P):
            if P == cv.zero:
                return cv.zero
            if (k, P) not in memo:
                memo[(k, P)] = cv.scale(k, P)
            return memo[(k, P)]

        # generic scalars; a + b = q (B = A sums to the identity, the accumulator passes through it on the way); a = b (B = -A
        # sums to the identity, with B = A the accumulator equals its addend); and the same through the shortcuts
        for a, b in ((s[0], s[1]), (s[0], q - s[0]), (s[1], s[1]), (1, q - 1), (1, 1)):
            ctx.points_lincomb(a, b, src_a=sa, src_b=sb, count=n, dst=f.sd)
            exp = [f.add(scale(a, P), scale(b, Q)) for P, Q in pairs]
            assert f.rows(f.sd, 0, n) == cv.wire(exp), (f.name, a, b)
            if (a + b) % q == 0:
                assert exp[4] == cv.zero and exp[12] == cv.zero
        ctx.pointset_select(f.sd)
        ctx.validate_points(0, n, "curve")
    finally:
        ctx.pointset_select(f.sa)
        ctx.pointset_destroy(sa)
        ctx.pointset_destroy(sb)


# ---------------------------------------------------------------------------------------------- 4: in place

@pytest.mark.parametrize("name", ["bls377", "ed377"])
def test_fold_in_place(name):
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError
    from montgomery_amd.api import MsmContext

    cv = D.CURVE_TABLE[name]
    q, n = cv.q, 642
    ctx = MsmContext(cv.cid)
    try:
        logs = O.scalars_from_bytes(ctx.generate_points(n, seed=1403, want_scalars=True))
        a, b = [v or 1 for v in _ints(f"{name}/fold", 2, q)]
        before = ctx.get_points(0, n)
        with pytest.raises(MsmError) as e:                     # a source range that overlaps the rows written
            ctx.points_lincomb(a, b, a_lo=1, b_lo=n // 2, count=n // 2)
        assert e.value.code == MSM_ERR_ARG
        with pytest.raises(MsmError) as e:
            ctx.points_lincomb(a, b, a_lo=0, b_lo=n // 2 - 1, count=n // 2)
        assert e.value.code == MSM_ERR_ARG
        assert ctx.pointset_size() == n and ctx.get_points(0, n) == before
        assert ctx.fold_points(a, b) == n // 2
        assert ctx.pointset_size() == n // 2 == ctx.n_points
        exp = [cv.scale_g((a * logs[i] + b * logs[i + n // 2]) % q) for i in range(n // 2)]
        assert ctx.get_points(0, n // 2) == cv.wire(exp)
        with pytest.raises(MsmError):                          # the set is truncated: row n / 2 is gone
            ctx.get_points(n // 2, 1)
    finally:
        ctx.close()


def test_fold_drops_the_tables_of_its_set_only(f377):
    f, ctx, q, n = f377, f377.ctx, f377.q, 8192
    kept, work = ctx.pointset_create(), None
    try:
        ctx.generate_points(4096, seed=1404)
        assert ctx.precompute()[1] >= 2
        kept_tables = ctx.tables_info()
        work = ctx.pointset_create()
        ctx.generate_points(n, seed=1405)
        assert ctx.precompute()[1] >= 2
        t = _ints("fold/tables", n // 2, q)
        u = _ints("fold/u", 1, q)[0] or 3
        want, _ = ctx.run(O.scalars_to_bytes(t + [u * s % q for s in t]), no_tables=True)
        assert ctx.fold_points(1, u) == n // 2
        assert ctx._cur_set == work and ctx.tables_info() == (0, 0, 0) and ctx.pointset_size() == n // 2
        got, info = ctx.run(O.scalars_to_bytes(t), no_tables=True)
        assert got == want and not info["tables"]
        # a fold into another set: the current set and its tables stay, and so do the tables of the set that is read
        ctx.pointset_select(kept)
        ctx.points_lincomb(1, u, src_a=kept, a_lo=0, src_b=kept, b_lo=2048, count=2048, dst=work)
        assert ctx._cur_set == kept and ctx.tables_info() == kept_tables and ctx.pointset_size() == 4096
        assert ctx.pointset_size(work) == 2048
        t2 = t[:2048]
        want2, info2 = ctx.run(O.scalars_to_bytes(t2 + [u * s % q for s in t2]))
        assert info2["tables"]
        got2, _ = f.run_on(work, t2)
        assert got2 == want2
    finally:
        ctx.pointset_select(f.sa)
        ctx.pointset_destroy(kept)
        if work is not None:
            ctx.pointset_destroy(work)


# ---------------------------------------------------------------------------------------------- 5: a whole IPA collapse

@pytest.mark.parametrize("name", ["pallas", "bn254", "ed377"])
def test_ipa_generator_collapse(name):
    """Ten in-place rounds over 1 024 generators.  Round j pairs row i with row i + n_j / 2, that is, it consumes bit
    log2(n) - 1 - j of the original index: the last point is sum_i s_i P_i with s_i = prod_j (hi_j if that bit of i is set else
    lo_j)."""
    from montgomery_amd.api import MsmContext

    cv = D.CURVE_TABLE[name]
    q, n, rounds = cv.q, 1024, 10
    ctx = MsmContext(cv.cid)
    try:
        orig = 0
        ctx.generate_points(n, seed=1406)
        work, prev = ctx.pointset_create(), ctx.pointset_create()
        ctx.points_lincomb(1, src_a=orig, dst=work)
        assert ctx.pointset_size(work) == n
        ch = [v or 2 for v in _ints(f"{name}/ipa", 2 * rounds, q)]
        lo, hi = ch[:rounds], ch[rounds:]
        lo[0] = 1                                              # Halo2's fold (1, u)
        lo[1] = pow(hi[1], -1, q)                              # Bulletproofs' fold (u^-1, u)
        m = n
        for j in range(rounds):
            ctx.points_lincomb(1, src_a=work, dst=prev)        # the kept copy of this round's input
            ctx.pointset_select(work)
            m //= 2
            assert ctx.fold_points(lo[j], hi[j]) == m
            t = _ints(f"{name}/ipa/t{j}", m, q)
            got, _ = ctx.run(O.scalars_to_bytes(t))
            ctx.pointset_select(prev)
            want, _ = ctx.run(O.scalars_to_bytes([lo[j] * s % q for s in t] + [hi[j] * s % q for s in t]))
            assert got == want, (name, j)
        s = []
        for i in range(n):
            v = 1
            for j in range(rounds):
                v = v * (hi[j] if (i >> (rounds - 1 - j)) & 1 else lo[j]) % q
            s.append(v)
        ctx.pointset_select(orig)
        want, _ = ctx.run(O.scalars_to_bytes(s))
        ctx.pointset_select(work)
        assert ctx.pointset_size() == 1
        last = ctx.get_point(0)
        assert last == ((want.x, want.y) if cv.te else want.as_tuple())
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 6: tables on a produced set

def test_window_tables_on_a_produced_set(f377):
    f, ctx, q, n = f377, f377.ctx, f377.q, 4096
    src, dst = ctx.pointset_create(), None
    try:
        logs = O.scalars_from_bytes(ctx.generate_points(2 * n, seed=1407, want_scalars=True))
        dst = ctx.pointset_create()
        a, b = [v or 1 for v in _ints("tables/ab", 2, q)]
        ctx.points_lincomb(a, b, src_a=src, a_lo=0, src_b=src, b_lo=n, count=n, dst=dst)
        assert ctx._cur_set == dst and ctx.n_points == n and ctx.tables_info() == (0, 0, 0)
        assert ctx.precompute()[1] >= 2
        t = _ints("tables/t", n, q)
        on_tables, info = ctx.run(O.scalars_to_bytes(t))
        plain, info_plain = ctx.run(O.scalars_to_bytes(t), no_tables=True)
        assert info["tables"] and not info_plain["tables"] and on_tables == plain
        exp = f.cv.scale_g(sum(s * (a * logs[i] + b * logs[n + i]) for i, s in enumerate(t)) % q)
        assert f.point(plain) == exp
    finally:
        ctx.pointset_select(f.sa)
        ctx.pointset_destroy(src)
        if dst is not None:
            ctx.pointset_destroy(dst)


# ---------------------------------------------------------------------------------------------- 7: errors

def test_every_refusal_leaves_the_context_usable(f7):
    from montgomery_amd._lib import MSM_ERR_ARG, MSM_ERR_NO_POINTS, MSM_ERR_SCALAR, MSM_OK, MsmError
    from montgomery_amd.api import MsmContext

    f, cv, q, ctx = f7, f7.cv, f7.q, f7.ctx
    lib, h = ctx._lib, ctx._h
    one = (ctypes.c_uint8 * 32)(1)
    ctx.points_lincomb(1, src_a=f.sa, count=65, dst=f.sd)
    before = f.rows(f.sd, 0, 65)

    def still_good():
        assert ctx.pointset_size(f.sd) == 65 and f.rows(f.sd, 0, 65) == before and ctx.pointset_size(f.sa) == N7
        ctx.points_lincomb(1, src_a=f.sa, count=65, dst=f.sd)          # and a call succeeds
        assert f.rows(f.sd, 0, 65) == before

    dead = ctx.pointset_create()
    ctx.pointset_destroy(dead)
    ctx.pointset_select(f.sa)
    bad = [
        (MSM_ERR_ARG, dict(src_a=99, count=1, dst=f.sd)), (MSM_ERR_ARG, dict(src_a=f.sa, count=1, dst=99)),
        (MSM_ERR_ARG, dict(src_a=dead, count=1, dst=f.sd)), (MSM_ERR_ARG, dict(src_a=f.sa, count=1, dst=-1)),
        (MSM_ERR_ARG, dict(src_a=f.sa, count=1 << 30, dst=f.sd)),
        (MSM_ERR_NO_POINTS, dict(src_a=f.sa, a_lo=N7 - 3, count=4, dst=f.sd)),
    ]
    for code, kw in bad:
        with pytest.raises(MsmError) as e:
            ctx.points_lincomb(5, **kw)
        assert e.value.code == code, kw
        still_good()
    for code, args in ((MSM_ERR_ARG, (5, 7, dict(src_a=f.sa, src_b=99, count=1, dst=f.sd))),
                       (MSM_ERR_NO_POINTS, (5, 7, dict(src_a=f.sa, src_b=f.sb, b_lo=N7, count=1, dst=f.sd))),
                       (MSM_ERR_SCALAR, (q, 7, dict(src_a=f.sa, src_b=f.sb, count=1, dst=f.sd))),
                       (MSM_ERR_SCALAR, (5, q, dict(src_a=f.sa, src_b=f.sb, count=1, dst=f.sd))),
                       (MSM_ERR_SCALAR, ((1 << 256) - 1, None, dict(src_a=f.sa, count=1, dst=f.sd)))):
        with pytest.raises(MsmError) as e:
            ctx.points_lincomb(args[0], args[1], **args[2])
        assert e.value.code == code, args
        still_good()
    # null scalars, at the C ABI
    assert lib.msm_points_lincomb(h, f.sa, 0, None, -1, 0, None, 1, f.sd) == MSM_ERR_ARG
    still_good()
    assert lib.msm_points_lincomb(h, f.sa, 0, one, f.sb, 0, None, 1, f.sd) == MSM_ERR_ARG
    still_good()
    assert lib.msm_points_lincomb(h, f.sa, 0, one, -1, 12345, None, 65, f.sd) == MSM_OK    # b and b_lo are ignored without a second term
    n_out = ctypes.c_uint64()
    assert lib.msm_pointset_size(h, 99, ctypes.byref(n_out)) == MSM_ERR_ARG
    assert lib.msm_pointset_size(h, dead, ctypes.byref(n_out)) == MSM_ERR_ARG
    still_good()
    # count == 0 is valid and leaves dst empty
    assert ctx.points_lincomb(5, 7, src_a=f.sa, src_b=f.sb, count=0, dst=f.sd) == 0
    assert ctx.pointset_size(f.sd) == 0
    ctx.points_lincomb(1, src_a=f.sa, count=65, dst=f.sd)
    assert f.rows(f.sd, 0, 65) == before
    # a device-list context
    multi = MsmContext(cv.cid, devices=[0, 0])
    try:
        multi.generate_points(8, seed=3)
        with pytest.raises(MsmError) as e:
            multi.points_lincomb(5)
        assert e.value.code == MSM_ERR_ARG
        assert len(multi.get_points(0, 8)) == 8 * f.step
    finally:
        multi.close()


# ---------------------------------------------------------------------------------------------- 8: launch geometry

def test_many_blocks_with_a_ragged_tail(f377):
    f, ctx, cv, q, n = f377, f377.ctx, f377.cv, f377.q, (1 << 16) + 1
    ids = []
    try:
        for _ in range(4):
            ids.append(ctx.pointset_create())
        sa, sb, sd, both = ids
        ctx.pointset_select(sa)
        la = O.scalars_from_bytes(ctx.generate_points(n, seed=1408, want_scalars=True))
        wa = ctx.get_points(0, n)
        ctx.pointset_select(sb)
        lb = O.scalars_from_bytes(ctx.generate_points(n, seed=1409, want_scalars=True))
        wb = ctx.get_points(0, n)
        ctx.pointset_select(both)
        ctx.set_points(wa + wb)
        a, b = [v or 1 for v in _ints("big/ab", 2, q)]
        ctx.points_lincomb(a, b, src_a=sa, src_b=sb, count=n, dst=sd)
        assert ctx.pointset_size(sd) == n and ctx._cur_set == both
        _, tb = ctx.generate_scalars(n, seed=1410, to_host=True)
        t = O.scalars_from_bytes(tb)
        want, _ = ctx.run(O.scalars_to_bytes([a * s % q for s in t] + [b * s % q for s in t]))
        got, _ = f.run_on(sd, t)
        assert got == want
        for i in (0, (1 << 16) - 1, 1 << 16):
            assert f.points(sd, i, 1) == [cv.scale_g((a * la[i] + b * lb[i]) % q)], i
    finally:
        ctx.pointset_select(f.sa)
        for i in ids:
            ctx.pointset_destroy(i)
