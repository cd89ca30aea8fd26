"""msm_scalars_ntt on the GPU, bit for bit against tests/ntt_model.py (Python integers).  `-m gpu`.

Every vector sits at an odd 32-byte offset inside its allocation with sentinel elements before and after; inputs carry q, q + 1,
2^256 - 1 and 0 among the random values, and the sources are read back unchanged.  The arithmetic is exact: no tolerances."""
import ctypes
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402
import ntt_model as M  # noqa: E402
import operator_fixture as F  # noqa: E402
from host_lib import host_library  # noqa: E402
from operator_fixture import SENTINEL, TOP, OperatorFixture, to_bytes  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

TWO_ADIC = ("bls377", "bls381", "pallas", "vesta", "bn254")


def _ints(tag, n, bound):
    return O.prng_ints(f"ntt/{tag}", n, bound)


def mixed(cv, tag, n):
    """operator_fixture.mixed, with a special element in a vector of up to three too"""
    return F.mixed("ntt", cv, tag, n, start=3 if n > 3 else 0)


def tiled(cv, tag, n, period=4093):
    """n elements that repeat `period` mixed ones: large vectors without a large generator run"""
    base = mixed(cv, tag, min(period, n))
    return [base[i % len(base)] for i in range(n)]


class Fix(OperatorFixture):
    def batch(self, vectors, pad=3):
        """the vectors of a batch back to back, as msm_scalars_ntt reads them, with the sentinels of vector() around the whole"""
        return self.vector([v for vec in vectors for v in vec], pad)

    def last_plan(self):
        return self.last("msm_test_last_ntt_plan", 32)

    def set_tile_log(self, t):
        self.set("msm_test_set_ntt_tile_log", t)


@pytest.fixture(scope="module", params=D.NAMES)
def f7(request):
    f = Fix(request.param)
    yield f
    f.close()


@pytest.fixture(scope="module")
def f377():
    f = Fix("bls377")
    yield f
    f.close()


@pytest.fixture(scope="module", params=["bls377", "bn254"])
def f2(request):
    f = Fix(request.param)
    yield f
    f.close()


@pytest.fixture(scope="module")
def default_tile_log():
    return host_library("ntt_host").ntt_default_tile_log()


def variants(q, log2n, tag):
    """(omega, shift, inverse) for the eight variants of a size; omega None = the library's root, else its cube"""
    root = M.root_of_unity(q, log2n)
    shift = _ints(f"{tag}/shift/{log2n}", 1, q - 1)[0] + 1
    return [(om, sh, inv) for om in (None, pow(root, 3, q)) for sh in (None, shift) for inv in (False, True)]


def model(vectors, q, log2n, omega, shift, inverse):
    om = M.root_of_unity(q, log2n) if omega is None else omega
    return [M.ntt(v, q, om, shift or 1, inverse) for v in vectors]


# ---------------------------------------------------------------------------------------------- 1: every size against the model

def test_every_size_against_the_model(f7, default_tile_log):
    f, q, ctx = f7, f7.q, f7.ctx
    top = ctx.scalars_ntt_max_log2n()
    assert top == M.max_log2n(q)
    assert (f.name in TWO_ADIC) == (top >= 12)
    for log2n in range(0, min(top, 12) + 1):
        n = 1 << log2n
        assert ctx.scalars_root_of_unity(log2n) == M.root_of_unity(q, log2n)
        vecs = [mixed(f.cv, f"size/{log2n}/{b}", n) for b in range(3)]
        a = f.batch(vecs)
        for omega, shift, inv in variants(q, log2n, f.name):
            exp = model(vecs, q, log2n, omega, shift, inv)
            for B in (1, 3):
                d = f.vector(B * n)
                ctx.scalars_ntt(d, a, log2n, inverse=inv, omega=omega, shift=shift, batch=B)
                assert f.read(d, B * n) == [v for vec in exp[:B] for v in vec], (f.name, log2n, omega is None, shift is None, inv, B)
                assert f.fenced(d, B * n), (f.name, log2n, B)
                plan = f.last_plan()
                assert sum(plan) == log2n and len(plan) == -(-log2n // default_tile_log), (log2n, plan)
                f.free(d)
        assert f.read(a, 3 * n) == [v for vec in vecs for v in vec] and f.fenced(a, 3 * n)      # the sources are as they were
        f.free(a)


# ---------------------------------------------------------------------------------------------- 2: pass boundaries at small sizes

def test_pass_boundaries_at_small_sizes(f2):
    f, q, ctx = f2, f2.q, f2.ctx
    try:
        for log2n in range(1, 13):
            n = 1 << log2n
            vecs = [mixed(f.cv, f"pass/{log2n}/{b}", n) for b in range(2)]
            a = f.batch(vecs)
            shift = _ints(f"{f.name}/pass/shift/{log2n}", 1, q - 1)[0] + 1
            for inv, sh in ((False, None), (True, None), (False, shift), (True, shift)):
                f.set_tile_log(0)
                ref = f.vector(2 * n)
                ctx.scalars_ntt(ref, a, log2n, inverse=inv, shift=sh, batch=2)
                want = f.read(ref, 2 * n)
                if (inv, sh) == (False, None):
                    assert want == [v for vec in model(vecs, q, log2n, None, sh, inv) for v in vec], (f.name, log2n, inv)
                f.free(ref)
                for tile_log in (2, 3, 5):
                    f.set_tile_log(tile_log)
                    d = f.vector(2 * n)
                    ctx.scalars_ntt(d, a, log2n, inverse=inv, shift=sh, batch=2)
                    plan = f.last_plan()
                    assert len(plan) == -(-log2n // tile_log) and sum(plan) == log2n and max(plan) <= tile_log, (log2n, tile_log, plan)
                    assert f.read(d, 2 * n) == want, (f.name, log2n, tile_log, inv, sh is not None)
                    assert f.fenced(d, 2 * n)
                    f.free(d)
            assert f.read(a, 2 * n) == [v for vec in vecs for v in vec]
            f.free(a)
        # one to six passes were all seen: 12 stages at tile_log 2 are six passes, 7 stages at 3 are a ragged 3 + 2 + 2
        f.set_tile_log(3)
        a = f.vector(mixed(f.cv, "pass/ragged", 128))
        ctx.scalars_ntt(a, a, 7)
        assert f.last_plan() == [3, 2, 2]
    finally:
        f.set_tile_log(0)


# ---------------------------------------------------------------------------------------------- 3: the default plan's own boundaries

def test_default_plan_boundaries(f377, default_tile_log):
    """log2n = T, T + 1, 2 T, 2 T + 1 for the default T: one pass, the first two-pass size, two full passes, the first three-pass
    size.  The round trip is compared over the whole vector; six outputs are checked as polynomial evaluations through
    scalars_powers and scalars_inner, which know nothing of the transform."""
    f, q, ctx, T = f377, f377.q, f377.ctx, default_tile_log
    assert 2 * T + 1 <= 23
    for log2n in (T, T + 1, 2 * T, 2 * T + 1):
        n = 1 << log2n
        A = tiled(f.cv, f"default/{log2n}", n)
        a, ev, back, pw = f.vector(A), f.vector(n), f.vector(n), f.vector(n)
        shift = _ints(f"default/shift/{log2n}", 1, q - 1)[0] + 1
        omega = ctx.scalars_root_of_unity(log2n)
        for sh in (None, shift):
            ctx.scalars_ntt(ev, a, log2n, shift=sh)
            assert len(f.last_plan()) == -(-log2n // T) and sum(f.last_plan()) == log2n
            ks = [0, 1, n // 2, n - 1] + _ints(f"default/k/{log2n}", 2, n)
            for k in ks:
                ctx.scalars_powers(pw, (sh or 1) * pow(omega, k, q) % q, n)
                assert f.read(ev + 32 * k, 1) == [ctx.scalars_inner(a, pw, n)], (log2n, k, sh is not None)
            ctx.scalars_ntt(back, ev, log2n, inverse=True, shift=sh)
            assert ctx.device_download(back, 32 * n) == to_bytes([v % q for v in A]), (log2n, sh is not None)
        assert ctx.device_download(a, 32 * n) == to_bytes(A)
        assert f.fenced(ev, n) and f.fenced(back, n)
        for p in (a, ev, back, pw):
            f.free(p)


# ---------------------------------------------------------------------------------------------- 4: in place

def test_in_place(f2, default_tile_log):
    f, q, ctx = f2, f2.q, f2.ctx
    try:
        for tile_log, log2n in ((0, 6), (0, 10), (3, 10), (2, 5)):
            f.set_tile_log(tile_log)
            n = 1 << log2n
            shift = _ints(f"{f.name}/inplace/shift", 1, q - 1)[0] + 1
            for B in (1, 3):
                vecs = [mixed(f.cv, f"inplace/{log2n}/{b}", n) for b in range(B)]
                for inv, sh in ((False, None), (True, shift)):
                    src, d, io = f.batch(vecs), f.vector(B * n), f.batch(vecs)
                    ctx.scalars_ntt(d, src, log2n, inverse=inv, shift=sh, batch=B)
                    passes = len(f.last_plan())
                    ctx.scalars_ntt(io, io, log2n, inverse=inv, shift=sh, batch=B)
                    assert len(f.last_plan()) == passes and (passes > 1) == (tile_log != 0 or log2n > default_tile_log)
                    assert f.read(io, B * n) == f.read(d, B * n) == [v for vec in model(vecs, q, log2n, None, sh, inv) for v in vec]
                    assert f.fenced(io, B * n)
                    for p in (src, d, io):
                        f.free(p)
    finally:
        f.set_tile_log(0)


# ---------------------------------------------------------------------------------------------- 5: the twiddle cache

def test_cache_follows_omega_and_size(f2):
    f, q, ctx = f2, f2.q, f2.ctx
    la, lb = 9, 11
    A, Bv = mixed(f.cv, "cache/a", 1 << la), mixed(f.cv, "cache/b", 1 << lb)
    a, b, d = f.vector(A), f.vector(Bv), f.vector(1 << lb)
    wa, wb = M.root_of_unity(q, la), M.root_of_unity(q, lb)
    wa3 = pow(wa, 3, q)
    exp_a, exp_a3, exp_b = M.ntt(A, q, wa), M.ntt(A, q, wa3), M.ntt(Bv, q, wb)
    # two roots at one size, then the first again (once by its value, once as the library's)
    for omega, exp in ((None, exp_a), (wa3, exp_a3), (wa, exp_a), (None, exp_a), (wa3, exp_a3)):
        ctx.scalars_ntt(d, a, la, omega=omega)
        assert f.read(d, 1 << la) == exp
    # two sizes in turn, and a direction change on cached tables
    for log2n, src, exp in ((lb, b, exp_b), (la, a, exp_a), (lb, b, exp_b)):
        ctx.scalars_ntt(d, src, log2n)
        assert f.read(d, 1 << log2n) == exp
        ctx.scalars_ntt(d, d, log2n, inverse=True)
        assert f.read(d, 1 << log2n) == [v % q for v in (Bv if log2n == lb else A)]


# ---------------------------------------------------------------------------------------------- 6: refusals

def test_every_refusal_leaves_the_context_usable(f7):
    from montgomery_amd._lib import MSM_ERR_ARG, MSM_ERR_SCALAR, MsmError

    f, q, ctx = f7, f7.q, f7.ctx
    lib, h = ctx._lib, ctx._h
    top = ctx.scalars_ntt_max_log2n()
    log2n = min(top, 6)
    n = 1 << log2n
    A = mixed(f.cv, "bad/a", 3 * n)
    a, d = f.vector(A), f.vector(3 * n)
    good = [v for b in range(2) for v in M.ntt(A[b * n:(b + 1) * n], q)]

    def still_good():
        assert f.read(a, 3 * n) == A and ctx.device_download(d, 32 * 3 * n) == SENTINEL * (3 * n)      # nothing was written
        t = f.vector(2 * n)
        ctx.scalars_ntt(t, a, log2n, batch=2)                                                           # and a call succeeds
        assert f.read(t, 2 * n) == good
        f.free(t)

    def refused(code, *args, **kw):
        with pytest.raises(MsmError) as e:
            ctx.scalars_ntt(*args, **kw)
        assert e.value.code == code, (args, kw)
        assert f.last_plan() == []
        still_good()
        return str(e.value)

    # partial overlap: one element up, one element down, half a vector, the last element of a batch
    refused(MSM_ERR_ARG, a + 32, a, log2n)
    refused(MSM_ERR_ARG, a, a + 32, log2n)
    refused(MSM_ERR_ARG, a + 16 * n, a, log2n, batch=2)
    refused(MSM_ERR_ARG, a + 32 * (2 * n - 1), a, log2n, batch=2)
    # misaligned pointers
    refused(MSM_ERR_ARG, d + 8, a, log2n)
    refused(MSM_ERR_ARG, d, a + 4, log2n)
    # B == 0, B n >= 2^30
    refused(MSM_ERR_ARG, d, a, log2n, batch=0)
    refused(MSM_ERR_ARG, d, a, log2n, batch=(1 << 30) >> log2n)
    # log2n beyond the curve's maximum, and beyond every maximum
    refused(MSM_ERR_ARG, d, a, top + 1)
    refused(MSM_ERR_ARG, d, a, 30)
    if f.name == "grumpkin":
        assert top == 1
        refused(MSM_ERR_ARG, d, a, 2)
    if f.name == "bn254":
        assert top == 28
        refused(MSM_ERR_ARG, d, a, 29)
    with pytest.raises(MsmError):
        ctx.scalars_root_of_unity(M.two_adicity(q) + 1)
    # omega of the wrong order: n / 2 and (where q - 1 has the factor) 2 n; the message says so
    w = M.root_of_unity(q, log2n)
    assert "order" in refused(MSM_ERR_ARG, d, a, log2n, omega=w * w % q)
    if log2n + 1 <= M.two_adicity(q):
        assert "order" in refused(MSM_ERR_ARG, d, a, log2n, omega=M.root_of_unity(q, log2n + 1))
    assert "order" in refused(MSM_ERR_ARG, d, a, log2n, omega=0)
    # host scalars at and above q; shift = 0
    refused(MSM_ERR_SCALAR, d, a, log2n, omega=q)
    refused(MSM_ERR_SCALAR, d, a, log2n, omega=TOP)
    refused(MSM_ERR_SCALAR, d, a, log2n, shift=q)
    refused(MSM_ERR_SCALAR, d, a, log2n, shift=q + 1, inverse=True)
    refused(MSM_ERR_ARG, d, a, log2n, shift=0)
    refused(MSM_ERR_ARG, d, a, log2n, shift=0, inverse=True)
    # null pointers, at the C ABI
    vp = ctypes.c_void_p
    for rc in (lib.msm_scalars_ntt(h, None, vp(a), log2n, 1, None, None, 0), lib.msm_scalars_ntt(h, vp(d), None, log2n, 1, None, None, 0)):
        assert rc == MSM_ERR_ARG
        still_good()
    assert lib.msm_scalars_ntt(None, vp(d), vp(a), log2n, 1, None, None, 0) == MSM_ERR_ARG
    out = (ctypes.c_uint8 * 32)()
    assert lib.msm_scalars_root_of_unity(None, 1, out) == MSM_ERR_ARG and lib.msm_scalars_root_of_unity(h, 1, None) == MSM_ERR_ARG
    assert lib.msm_scalars_ntt_max_log2n(h, None) == MSM_ERR_ARG
    # for n = 1 omega is ignored, whatever it holds
    ctx.scalars_ntt(d, a, 0, omega=TOP)
    assert f.read(d, 1) == [A[0] % q]


def test_device_list_contexts_are_refused():
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError
    from montgomery_amd.api import MsmContext

    multi = MsmContext(D.CURVE_TABLE["bls377"].cid, devices=[0, 0])
    try:
        p = multi.device_alloc(128)
        multi.device_upload(p, bytes(128))
        with pytest.raises(MsmError) as e:
            multi.scalars_ntt(p + 64, p, 1)
        assert e.value.code == MSM_ERR_ARG
        assert multi._lib.msm_test_set_ntt_tile_log(multi._h, 3) == MSM_ERR_ARG
        assert multi._lib.msm_test_last_ntt_plan(multi._h, None, 0) == -1
        assert multi.device_download(p, 128) == bytes(128)
    finally:
        multi.close()


# ---------------------------------------------------------------------------------------------- 7: end to end

@pytest.mark.parametrize("name", TWO_ADIC)
def test_polynomial_product(name):
    """iNTT(NTT(a) o NTT(b)) is the schoolbook product of two polynomials of degree < 128, at n = 256"""
    f = Fix(name)
    try:
        q, ctx, n = f.q, f.ctx, 256
        A, Bc = _ints(f"{name}/prod/a", 128, q), _ints(f"{name}/prod/b", 128, q)
        a, b = f.vector(A + [0] * 128), f.vector(Bc + [0] * 128)
        ctx.scalars_ntt(a, a, 8)
        ctx.scalars_ntt(b, b, 8)
        ctx.scalars_mul(a, a, b, n)
        ctx.scalars_ntt(a, a, 8, inverse=True)
        prod = [0] * n
        for i, u in enumerate(A):
            for j, v in enumerate(Bc):
                prod[i + j] = (prod[i + j] + u * v) % q
        assert f.read(a, n) == prod
    finally:
        f.close()


def test_evaluations_to_commitment(f7):
    """evaluations -> scalars_ntt(inverse) -> msm_run over the device result, at 2^10 generated points (2 where q allows no more):
    the point is (sum coeff_i g_i) G by the known discrete logs"""
    f, cv, q, ctx = f7, f7.cv, f7.q, f7.ctx
    log2n = min(10, ctx.scalars_ntt_max_log2n())
    n = 1 << log2n
    logs = O.scalars_from_bytes(ctx.generate_points(n, seed=1601, want_scalars=True))
    E = mixed(cv, "commit/evals", n)
    ev = f.vector(E)
    ctx.scalars_ntt(ev, ev, log2n, inverse=True)
    coeffs = M.ntt(E, q, inverse=True)
    assert f.read(ev, n) == coeffs
    got, _ = ctx.run_device(ev, n)
    assert f.point(got) == cv.scale_g(sum(c * g for c, g in zip(coeffs, logs)) % q)
