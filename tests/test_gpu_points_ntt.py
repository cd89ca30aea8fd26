"""msm_points_ntt: the transform D[k] = sum_j (shift omega^k)^j A[j] over the rows of a point set, and its inverse, on the GPU.
`-m gpu`.

The fixture is that of tests/test_gpu_points_lincomb.py: sets of 336 generated points with known logs (P_j = d_j G), so a produced
row has the expected value E_k G from the oracle, E = the transform of d in Python integers mod q.  The five curves whose q - 1
has two-adicity above 1 run log2n = 0 .. 8; Grumpkin and Ed-on-BLS12-377 run log2n = 0, 1 and refuse 2.  The larger transforms
(2^10 rows, which take two blocks, so forced grids of one to three blocks differ from the default) are compared row for row with
msm_points_mul_base over the transformed scalars."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degenerate_inputs as D  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402
from test_gpu_points_lincomb import N7, Fix  # noqa: E402

pytestmark = pytest.mark.gpu
TWO_ADIC = ("bls377", "bls381", "pallas", "bn254", "vesta")
ONE_ADIC = ("grumpkin", "ed377")
BIG_LOG = 10


def _ints(tag, n, bound):
    return O.prng_ints(f"points_ntt/{tag}", n, bound)


def sbytes(scalars):
    return b"".join(int(s).to_bytes(32, "little") for s in scalars)


def last_plan(ctx):
    """(log2n, butterfly launches, grid blocks, multiplication-free launches, pre-scaling, post-scaling, butterflies with a
    twiddle other than 1) of the last msm_points_ntt, from the library's own report"""
    out = (ctypes.c_int32 * 7)()
    assert ctx._lib.msm_test_last_points_ntt(ctx._h, out, 7) == 7
    return tuple(out)


def set_grid(ctx, blocks):
    ctx._check(ctx._lib.msm_test_set_points_ntt_grid(ctx._h, blocks))


def derived_plan(cv, L, shifted, inverse, blocks=None):
    """what the header documents for a transform of 2^L rows"""
    if blocks is None:
        blocks = 0 if (L == 0 or cv.te) else -(-(1 << (L - 1)) // 256)
    muls = ((1 << (L - 1)) * (L - 2) + 1) if L >= 2 else 0
    return (L, L, blocks, int(L >= 1), int(L >= 1 and shifted and not inverse), int(L >= 1 and inverse), muls)


def transform(d, L, om, shift, inverse, q):
    """the documented map over Python integers mod q (n <= 2^10: the plain double sum over a table of powers)"""
    n = 1 << L
    if not inverse:
        a = [v * pow(shift, j, q) % q for j, v in enumerate(d)]
        w = [pow(om, e, q) for e in range(n)]
        return [sum(a[j] * w[j * k % n] for j in range(n)) % q for k in range(n)]
    omi, ni, si = pow(om, -1, q), pow(n, -1, q), pow(shift, -1, q)
    w = [pow(omi, e, q) for e in range(n)]
    return [sum(d[k] * w[j * k % n] for k in range(n)) * ni * pow(si, j, q) % q for j in range(n)]


def roots(ctx, L, q):
    """the library's root of 2^L and another primitive one"""
    lib_root = ctx.scalars_root_of_unity(L)
    return lib_root, pow(lib_root, 3, q)


@pytest.fixture(scope="module", params=D.NAMES)
def f7(request):
    f = Fix(request.param)
    yield f
    f.ctx.close()


def check_case(f, L, inverse, own_root, shifted, a_lo):
    cv, q, ctx = f.cv, f.q, f.ctx
    n = 1 << L
    lib_root, other = roots(ctx, L, q)
    om = other if own_root else lib_root
    shift = (_ints(f"{f.name}/shift/{L}", 1, q)[0] | 2) if shifted else 1
    assert ctx.points_ntt(src=f.sa, a_lo=a_lo, log2n=L, omega=om if own_root else None, shift=shift if shifted else None,
                          inverse=inverse, dst=f.sd) == n
    assert last_plan(ctx) == derived_plan(cv, L, shifted, inverse), (f.name, L, inverse, own_root, shifted, a_lo)
    assert ctx.pointset_size(f.sd) == n and ctx._cur_set == f.sa and ctx.pointset_size() == N7
    E = transform(f.la[a_lo:a_lo + n], L, om, shift, inverse, q)
    assert f.rows(f.sd, 0, n) == cv.wire([cv.scale_g(e) for e in E]), (f.name, L, inverse, own_root, shifted, a_lo)
    return E


# ---------------------------------------------------------------------------------------------- 3: forward and inverse, 2^0 .. 2^8

ALL16 = [(inv, own, sh, a_lo) for inv in (False, True) for own in (False, True) for sh in (False, True) for a_lo in (0, 3)]
# four combinations in which every pair of choices meets (an orthogonal array of strength 2), and their complements
OA4 = [(False, False, False, 0), (False, True, True, 3), (True, False, True, 3), (True, True, False, 0)]
OA4C = [(not i, not o, not s, 3 - a) for i, o, s, a in OA4]


@pytest.mark.parametrize("L", range(0, 9))
def test_forward_and_inverse_against_the_oracle(f7, L):
    """log2n = 0 .. 2: all sixteen combinations of direction, root, shift and a_lo; 3 .. 6: eight that cover every pair of
    choices both ways; 7 and 8: two each (complementary in all four choices), the rest of their ground being the round trips."""
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError

    f = f7
    if f.name in ONE_ADIC and L > 1:                                         # transforms of one and two points only
        with pytest.raises(MsmError) as e:
            f.ctx.points_ntt(src=f.sa, log2n=L, dst=f.sd)
        assert e.value.code == MSM_ERR_ARG and f.ctx.pointset_size(f.sa) == N7
        return
    combos = ALL16 if L <= 2 else OA4 + OA4C if L <= 6 else [OA4[1 + L % 2], OA4C[1 + L % 2]]
    for inv, own, sh, a_lo in combos:
        check_case(f, L, inv, own, sh, a_lo)


@pytest.mark.parametrize("name", ONE_ADIC)
def test_log2n_2_is_refused(name):
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError
    from montgomery_amd.api import MsmContext

    cv = D.CURVE_TABLE[name]
    ctx = MsmContext(cv.cid)
    try:
        ctx.generate_points(8, seed=1601)
        before = ctx.get_points(0, 8)
        assert ctx.scalars_ntt_max_log2n() == 1
        with pytest.raises(MsmError) as e:
            ctx.points_ntt(log2n=2)
        assert e.value.code == MSM_ERR_ARG and "2^1" in str(e.value)
        assert ctx.pointset_size() == 8 and ctx.get_points(0, 8) == before and last_plan(ctx) == (0,) * 7
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 4, 5: 2^10 rows

class Big:
    """2^10 points d_j G on BLS12-377 from msm_points_mul_base, and the forward transform of d"""

    def __init__(self):
        from montgomery_amd.api import MsmContext

        self.cv = cv = D.CURVE_TABLE["bls377"]
        self.q, self.n = cv.q, 1 << BIG_LOG
        self.ctx = ctx = MsmContext(cv.cid)
        self.d = _ints("big/d", self.n, cv.q)
        self.src, self.dst, self.ref = 0, ctx.pointset_create(), ctx.pointset_create()
        ctx.pointset_select(self.src)
        ctx.points_mul_base(sbytes(self.d), dst=self.src)
        self.om = ctx.scalars_root_of_unity(BIG_LOG)
        self.step = 2 * ctx.coord_bytes

    def rows(self, set_id, first=0, count=None):
        ctx = self.ctx
        ctx.pointset_select(set_id)
        try:
            return ctx.get_points(first, self.n if count is None else count)
        finally:
            ctx.pointset_select(self.src)

    def reference_rows(self, E):
        """E_k G through msm_points_mul_base: code that shares nothing with the transform"""
        self.ctx.points_mul_base(sbytes(E), dst=self.ref)
        return self.rows(self.ref)


@pytest.fixture(scope="module")
def big():
    b = Big()
    b.E = transform(b.d, BIG_LOG, b.om, 1, False, b.q)
    b.want = b.reference_rows(b.E)
    yield b
    b.ctx.close()


def test_two_to_the_ten_forward_and_inverse_on_a_coset(big):
    b, ctx, cv, q, n = big, big.ctx, big.cv, big.q, big.n
    assert ctx.points_ntt(src=b.src, log2n=BIG_LOG, dst=b.dst) == n
    assert last_plan(ctx) == derived_plan(cv, BIG_LOG, False, False, blocks=2) and last_plan(ctx)[6] == 4097
    got = b.rows(b.dst)
    assert got == b.want
    sample = _ints("big/sample", 32, n)
    for k in sample:
        assert got[b.step * k:b.step * (k + 1)] == cv.wire([cv.scale_g(b.E[k])]), k
    shift = _ints("big/shift", 1, q)[0] | 2
    assert ctx.points_ntt(src=b.src, log2n=BIG_LOG, shift=shift, inverse=True, dst=b.dst) == n
    assert last_plan(ctx) == derived_plan(cv, BIG_LOG, True, True, blocks=2)
    Ei = transform(b.d, BIG_LOG, b.om, shift, True, q)
    got = b.rows(b.dst)
    assert got == b.reference_rows(Ei)
    for k in sample[:8]:
        assert got[b.step * k:b.step * (k + 1)] == cv.wire([cv.scale_g(Ei[k])]), k


def test_the_rows_do_not_depend_on_the_grid(big):
    """512 butterflies per stage: one block gives every lane two (the table slots are rebuilt), three blocks a ragged second
    stride; a workspace limit with room for one block's tables does what a forced grid of one does."""
    b, ctx = big, big.ctx
    try:
        for blocks in (1, 2, 3, 0):
            set_grid(ctx, blocks)
            ctx.points_ntt(src=b.src, log2n=BIG_LOG, dst=b.dst)
            assert last_plan(ctx)[2] == (blocks or 2)
            assert b.rows(b.dst) == b.want, blocks
    finally:
        set_grid(ctx, 0)
    per_block = 256 * 8 * 4 * ctx.coord_bytes              # lanes x entries (w = 4) x coordinates x bytes
    try:
        ctx.set_workspace_limit(per_block + per_block // 2)
        ctx.points_ntt(src=b.src, log2n=BIG_LOG, dst=b.dst)
        assert last_plan(ctx)[2] == 1
        assert b.rows(b.dst) == b.want
    finally:
        ctx.set_workspace_limit(0)


# ---------------------------------------------------------------------------------------------- 6: round trips

@pytest.mark.parametrize("shifted", (False, True))
def test_round_trips_in_place_and_inside_one_set(f7, shifted):
    f, cv, q, ctx = f7, f7.cv, f7.q, f7.ctx
    L = 1 if f.name in ONE_ADIC else 7
    n, a_lo = 1 << L, 200
    shift = (_ints(f"{f.name}/rt", 1, q)[0] | 2) if shifted else None
    src_rows = f.rows(f.sa, a_lo, n)
    work = ctx.pointset_create()
    ctx.pointset_select(f.sa)
    try:
        for first in (False, True):                                          # inverse(forward(A)), then forward(inverse(A))
            ctx.points_lincomb(1, src_a=f.sa, count=N7, dst=work)            # a copy of the 336 rows
            # out of place inside one set: the rows [a_lo, a_lo + n) -> the rows [0, n), the set truncated to n
            assert ctx.points_ntt(src=work, a_lo=a_lo, log2n=L, shift=shift, inverse=first, dst=work) == n
            assert ctx.pointset_size(work) == n
            E = transform(f.la[a_lo:a_lo + n], L, ctx.scalars_root_of_unity(L), shift or 1, first, q)
            assert f.points(work, 0, 2) == [cv.scale_g(E[0]), cv.scale_g(E[1])]
            # in place: the way back
            assert ctx.points_ntt(src=work, log2n=L, shift=shift, inverse=not first, dst=work) == n
            assert ctx.pointset_size(work) == n and f.rows(work, 0, n) == src_rows, (f.name, shifted, first)
            # and out of place into another set
            ctx.points_ntt(src=f.sa, a_lo=a_lo, log2n=L, shift=shift, inverse=first, dst=f.sd)
            ctx.points_ntt(src=f.sd, log2n=L, shift=shift, inverse=not first, dst=work)
            assert f.rows(work, 0, n) == src_rows
        assert ctx._cur_set == f.sa and ctx.pointset_size(f.sa) == N7
    finally:
        ctx.pointset_destroy(work)


# ---------------------------------------------------------------------------------------------- 7: degenerate sets

def stages(d, L, om, q, upto):
    """the rows' logs after the bit reversal and the stages 1 .. upto of the plan of points_ntt.h"""
    n = 1 << L
    x = [d[int(format(i, f"0{L}b")[::-1], 2)] for i in range(n)]
    for s in range(1, upto + 1):
        m, blocks = 1 << s, n >> s
        for t in range(n // 2):
            j, blk = t // blocks, t % blocks
            ia = blk * m + j
            ib = ia + m // 2
            wb = pow(om, j * blocks, q) * x[ib] % q
            x[ia], x[ib] = (x[ia] + wb) % q, (x[ia] - wb) % q
    return x


def crafted_logs(name, L, om, q):
    """Random logs, four of them solved so that A = w B at one butterfly of stage 2 and one of stage 3 and A = -w B at another of
    each, all with w != 1 and in different blocks, the other butterflies of their waves generic."""
    n = 1 << L
    d = [v | 1 for v in _ints(f"{name}/crafted", n, q)]
    spots = []                                                               # (stage, row a, row b, twiddle, sign)
    for s, blk, sign in ((2, 0, 1), (2, 1, -1), (3, 2, 1), (3, 3, -1)):
        m, blocks = 1 << s, n >> s
        j = m // 2 - 1
        ia = blk * m + j
        spots.append((s, ia, ia + m // 2, pow(om, j * blocks, q), sign))
    for s, ia, ib, w, sign in spots:
        # x[ia] before stage s is linear in the input that the bit reversal puts at row ia's first leaf; x[ib] does not read it
        leaf = int(format(ia & ~((1 << (s - 1)) - 1), f"0{L}b")[::-1], 2)
        d0, d1 = list(d), list(d)
        d0[leaf], d1[leaf] = 0, 1
        r0, r1 = stages(d0, L, om, q, s - 1), stages(d1, L, om, q, s - 1)
        assert r0[ib] == r1[ib]
        target = sign * w * r0[ib] % q
        d[leaf] = (target - r0[ia]) * pow(r1[ia] - r0[ia], -1, q) % q
    for s, ia, ib, w, sign in spots:
        x = stages(d, L, om, q, s - 1)
        assert x[ia] == sign * w * x[ib] % q and x[ia] != 0 and w != 1
    return d


@pytest.mark.parametrize("name", TWO_ADIC)
def test_degenerate_sets(name):
    from montgomery_amd.api import MsmContext

    cv = D.CURVE_TABLE[name]
    q, L = cv.q, 6
    n = 1 << L
    c = D.pool(name)[1][0]
    ctx = MsmContext(cv.cid)
    try:
        dst = ctx.pointset_create()
        ctx.pointset_select(0)
        om = ctx.scalars_root_of_unity(L)
        cases = {
            "all rows equal": [c] * n,                                       # stage 1 doubles and cancels in every butterfly
            "all identity": [0] * n,
            "one row": [0] * 5 + [c] + [0] * (n - 6),
            "A = +-w B at stages 2 and 3": crafted_logs(name, L, om, q),
        }
        for what, d in cases.items():
            ctx.points_mul_base(sbytes(d), dst=0)
            for inverse in (False, True):
                assert ctx.points_ntt(src=0, log2n=L, inverse=inverse, dst=dst) == n
                E = transform(d, L, om, 1, inverse, q)
                ctx.pointset_select(dst)
                got = ctx.get_points(0, n)
                ctx.pointset_select(0)
                assert got == cv.wire([cv.scale_g(e) for e in E]), (name, what, inverse)
                if what == "all rows equal" and not inverse:
                    assert E[1:] == [0] * (n - 1) and E[0] == n * c % q
                if what != "A = +-w B at stages 2 and 3":
                    break                                                    # (the inverse of these runs the same butterflies)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 8: monomial key -> Lagrange key

@pytest.mark.parametrize("name", ("bls377", "bn254"))
def test_lagrange_key_commits_to_evaluations(name):
    """[tau^j] G from scalars_powers + points_mul_base; its inverse transform is the key in the Lagrange basis: msm_run over the
    EVALUATIONS of f on that key equals msm_run over the coefficients of f on the monomial key.  On a coset the evaluation map
    M[k][j] = (shift omega^k)^j is not symmetric and the key that commits to M f is (M^T)^-1 A: 1 / n times the forward
    transform under omega^-1 and shift^-1 (include/msm_hip.h), row k = [L_k(tau)] G with L_k the Lagrange basis of the coset."""
    from montgomery_amd.api import MsmContext

    cv = D.CURVE_TABLE[name]
    q, L = cv.q, 8
    n = 1 << L
    ctx = MsmContext(cv.cid)
    try:
        tau = _ints(f"{name}/tau", 1, q)[0] | 2
        coeff = _ints(f"{name}/f", n, q)
        mono, lag = 0, ctx.pointset_create()
        ctx.pointset_select(mono)
        dev, ev = ctx.device_alloc(32 * n), ctx.device_alloc(32 * n)
        ctx.scalars_powers(dev, tau, n)
        ctx.points_mul_base(dev, count=n, dst=mono)
        commitment = cv.scale_g(sum(ci * pow(tau, i, q) for i, ci in enumerate(coeff)) % q)

        def point(res):
            return res.as_tuple()

        got, _ = ctx.run(sbytes(coeff))
        assert point(got) == commitment
        for shift in (None, _ints(f"{name}/coset", 1, q)[0] | 2):
            om = ctx.scalars_root_of_unity(L)
            if shift is None:
                assert ctx.points_ntt(src=mono, log2n=L, inverse=True, dst=lag) == n
                ctx.pointset_select(lag)
                by_inverse = ctx.get_points(0, n)
                ctx.pointset_select(mono)
            # the transpose inverse: forward under omega^-1 and shift^-1, then n^-1 on every row
            assert ctx.points_ntt(src=mono, log2n=L, omega=pow(om, -1, q), shift=None if shift is None else pow(shift, -1, q), dst=lag) == n
            assert ctx.points_lincomb(pow(n, -1, q), src_a=lag, count=n, dst=lag) == n
            ctx.device_upload(dev, sbytes(coeff))
            ctx.scalars_ntt(ev, dev, L, shift=shift)                         # the evaluations of f on shift <omega>
            evals = ctx.device_download(ev, 32 * n)
            ctx.pointset_select(lag)
            try:
                glv, _ = ctx.run(evals)
                plain, _ = ctx.run(evals, no_glv=True)
                assert point(glv) == commitment and point(plain) == commitment, (name, shift)
                ctx.precompute()
                tabled, _ = ctx.run(evals)
                assert point(tabled) == commitment
                # row k is L_k(tau) G, L_k(X) = (X^n - s^n) s omega^k / (n s^n (X - s omega^k)); without a shift the two routes
                # to the key write the same rows
                s = shift or 1
                for k in (0, 5):
                    x = s * pow(om, k, q) % q
                    lk = (pow(tau, n, q) - pow(s, n, q)) * x * pow(n * pow(s, n, q) * (tau - x), -1, q) % q
                    assert ctx.get_points(k, 1) == cv.wire([cv.scale_g(lk)]), (name, shift, k)
                if shift is None:
                    assert ctx.get_points(0, n) == by_inverse
            finally:
                ctx.pointset_select(mono)
        ctx.device_free(dev)
        ctx.device_free(ev)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 9: refusals

def test_every_refusal_leaves_the_sets_as_they_were(f7):
    from montgomery_amd._lib import MSM_ERR_ARG, MSM_ERR_NO_POINTS, MSM_ERR_SCALAR, MsmError
    from montgomery_amd.api import MsmContext

    f, cv, q, ctx = f7, f7.cv, f7.q, f7.ctx
    lib, h = ctx._lib, ctx._h
    L = 1 if f.name in ONE_ADIC else 3
    n = 1 << L
    ctx.points_ntt(src=f.sa, a_lo=16, log2n=4 if L == 3 else 1, dst=f.sd)
    kept = ctx.pointset_size(f.sd)
    before, src_before = f.rows(f.sd, 0, kept), f.rows(f.sa, 0, N7)

    def still_good():
        assert ctx.pointset_size(f.sd) == kept and f.rows(f.sd, 0, kept) == before
        assert ctx.pointset_size(f.sa) == N7 and f.rows(f.sa, 0, N7) == src_before
        assert last_plan(ctx) == (0,) * 7

    dead = ctx.pointset_create()
    ctx.pointset_destroy(dead)
    ctx.pointset_select(f.sa)

    def b32(v):
        return (ctypes.c_uint8 * 32).from_buffer_copy(int(v).to_bytes(32, "little"))

    root = ctx.scalars_root_of_unity(L)
    bad = [
        (MSM_ERR_ARG, (99, 0, L, None, None, 0, f.sd)), (MSM_ERR_ARG, (f.sa, 0, L, None, None, 0, 99)),
        (MSM_ERR_ARG, (dead, 0, L, None, None, 0, f.sd)), (MSM_ERR_ARG, (f.sa, 0, L, None, None, 0, -1)),
        (MSM_ERR_ARG, (f.sa, 0, ctx.scalars_ntt_max_log2n() + 1, None, None, 0, f.sd)),           # log2n too large
        (MSM_ERR_ARG, (f.sa, 0, L, b32(root * root % q), None, 0, f.sd)),                         # omega of half the order
        (MSM_ERR_ARG, (f.sa, 0, L, b32(1), None, 1, f.sd)),
        (MSM_ERR_SCALAR, (f.sa, 0, L, b32(q), None, 0, f.sd)), (MSM_ERR_SCALAR, (f.sa, 0, L, b32(q + root), None, 0, f.sd)),
        (MSM_ERR_ARG, (f.sa, 0, L, None, b32(0), 0, f.sd)), (MSM_ERR_ARG, (f.sa, 0, L, None, b32(0), 1, f.sd)),
        (MSM_ERR_SCALAR, (f.sa, 0, L, None, b32(q), 0, f.sd)), (MSM_ERR_SCALAR, (f.sa, 0, 0, None, b32(q + 1), 0, f.sd)),
        (MSM_ERR_NO_POINTS, (f.sa, N7 - n + 1, L, None, None, 0, f.sd)), (MSM_ERR_NO_POINTS, (f.sd, kept, 0, None, None, 0, f.sa)),
        (MSM_ERR_ARG, (f.sa, 1, L, None, None, 0, f.sa)), (MSM_ERR_ARG, (f.sa, n - 1, L, None, None, 1, f.sa)),   # forbidden overlaps
    ]
    for code, args in bad:
        assert lib.msm_points_ntt(h, *args) == code, args
        still_good()
    # for one point omega is not looked at
    assert lib.msm_points_ntt(h, f.sa, 5, 0, b32(q + 5), None, 0, f.sd) == 0
    assert ctx.pointset_size(f.sd) == 1 and f.rows(f.sd, 0, 1) == src_before[5 * f.step:6 * f.step]
    multi = MsmContext(cv.cid, devices=[0, 0])
    try:
        multi.generate_points(8, seed=3)
        with pytest.raises(MsmError) as e:
            multi.points_ntt(log2n=1)
        assert e.value.code == MSM_ERR_ARG
        assert len(multi.get_points(0, 8)) == 8 * f.step
    finally:
        multi.close()
