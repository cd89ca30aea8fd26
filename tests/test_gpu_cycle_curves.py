"""BN254 G1 (curve id 4), Grumpkin (5) and Vesta (6) on the GPU: `-m gpu`.

Operators against Python integers, MSMs against the committed oracle fixtures (tests/golden/cycles_*.json) and against the
known-discrete-log identity sum s_i P_i = (sum s_i a_i) G over generated points, and each inherited feature (batch, narrow
scalars, window sums and their combines, skew, compressed ingest, the Python facade) once per curve.  The CPU side is the
Python oracle run on parameters restated in tests/test_cycle_curves.py: oracle/ has no entry for these curves.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import msm_oracle as O  # noqa: E402
from test_cycle_curves import CURVES, NAMES, compress, decompress, limb_operands, packed_edge_values  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CB, NL = 32, 9
R = 1 << (30 * NL)
M30 = (1 << 30) - 1


def tb(v):
    return v.to_bytes(CB, "little")


def fb(b, i):
    return int.from_bytes(b[CB * i : CB * i + CB], "little")


def enc_pt(P):
    return b"\0" * (2 * CB) if P is None else tb(P[0]) + tb(P[1])


def dec_pt(b, i=0):
    x, y = fb(b, 2 * i), fb(b, 2 * i + 1)
    return None if (x, y) == (0, 0) else (x, y)


class Case:
    def __init__(self, name):
        from montgomery_amd.api import MsmContext

        self.name = name
        self.cid, self.B = CURVES[name][:2]
        self.pasta = CURVES[name][6]
        self.ctx = MsmContext(self.cid)     # msm_ctx_create: MSM_ERR_ARG before these curves existed
        with open(os.path.join(GOLD, f"cycles_{name}.json")) as f:
            self.gold = json.load(f)
        self.G = (self.B.gx, self.B.gy)

    def dlog_point(self, k):
        return O.aff_scale(k % self.B.q, self.G, self.B.p)


@pytest.fixture(scope="module", params=NAMES)
def cv(request):
    case = Case(request.param)
    assert case.ctx.coord_bytes == CB
    yield case
    case.ctx.close()


def run_msm(ctx, scalars, points, c=None, **kw):
    ctx.set_points(b"".join(enc_pt(P) for P in points), check_curve=True)
    res, info = ctx.run(O.scalars_to_bytes(scalars), c=c, **kw)
    return res.as_tuple(), info


def generated(cv, n, seed):
    """n points a_i G generated on the GPU (resident), device scalars s_i, and the expected sum."""
    from oracle import c_oracle

    a = cv.ctx.generate_points(n, seed=seed, want_scalars=True, raw=True)
    dev, s = cv.ctx.generate_scalars(n, seed=seed + 1, to_host=True, raw=True)
    return dev, s, cv.dlog_point(c_oracle.dot_mod(a, s, n, cv.B.q))


# ---------------------------------------------------------------------------------------------- the context, the ABI

def test_context_and_abi_version(cv):
    from montgomery_amd import _lib

    lib = _lib.load()
    assert lib.msm_abi_version() == 8
    assert cv.ctx.curve == cv.cid and cv.ctx.coord_bytes == 32
    assert cv.ctx.generate_points(4, seed=1, want_scalars=True) is not None
    a = O.scalars_from_bytes(cv.ctx.generate_points(4, seed=1, want_scalars=True))
    assert [cv.ctx.get_point(i) for i in range(4)] == [cv.dlog_point(k) for k in a]


def test_unknown_curve_id_is_still_refused():
    from montgomery_amd import MsmError
    from montgomery_amd.api import MsmContext

    for cid in (7, -1, 100):
        with pytest.raises(MsmError) as e:
            MsmContext(cid)
        assert e.value.code == 1


# ---------------------------------------------------------------------------------------------- operators

def test_fp_operators_and_four_inversions(cv):
    from montgomery_amd import _lib

    ctx, p = cv.ctx, cv.B.p
    vals = [0, 1, 2, p - 1, p - 2, (p + 1) // 2, 1 << (p.bit_length() - 1), (1 << 30) - 1, 1 << 30, (1 << 250) + 5] + \
        O.prng_ints(f"gpu/cycles/fp/{cv.name}", 500, p)
    n = len(vals)
    a = b"".join(tb(v) for v in vals)
    b = b"".join(tb(v) for v in reversed(vals))
    rinv = pow(R, -1, p)
    out = ctx.test_fp(_lib.OP_MUL, a, b)
    assert all(fb(out, i) == vals[i] * vals[n - 1 - i] * rinv % p for i in range(n))
    out = ctx.test_fp(_lib.OP_SQR, a)
    assert all(fb(out, i) == vals[i] * vals[i] * rinv % p for i in range(n))
    out = ctx.test_fp(_lib.OP_ADD, a, b)      # fe_add / fe_sub_p on 30-bit limbs (the packed chains: test_packed_chains_on_edge_operands)
    assert all(fb(out, i) == (vals[i] + vals[n - 1 - i]) % p for i in range(n))
    out = ctx.test_fp(_lib.OP_SUB, a, b)
    assert all(fb(out, i) == (vals[i] - vals[n - 1 - i]) % p for i in range(n))
    nz = [v for v in vals if v]
    an = b"".join(tb(v) for v in nz)
    mont = ctx.test_fp(_lib.OP_TO_MONT, an)
    assert all(fb(mont, i) == v * R % p for i, v in enumerate(nz))
    assert ctx.test_fp(_lib.OP_FROM_MONT, mont) == an
    inv = ctx.test_fp(_lib.OP_INV, mont)
    back = ctx.test_fp(_lib.OP_FROM_MONT, inv)
    assert all(fb(back, i) == pow(v, -1, p) for i, v in enumerate(nz))
    for op in (_lib.OP_INV_FERMAT, _lib.OP_INV_KALISKI, _lib.OP_INV_WORDSLICED):
        assert ctx.test_fp(op, mont[: CB * 64]) == inv[: CB * 64], op
    for per_lane in (1, 7, 100):
        out = ctx.test_fp(_lib.OP_FROM_MONT, ctx.test_batch_inverse(mont[: CB * 203], per_lane))
        assert all(fb(out, i) == pow(v, -1, p) for i, v in enumerate(nz[:203])), per_lane


def test_fp_raw_on_unreduced_and_all_ones_operands(cv):
    from montgomery_amd import _lib

    p = cv.B.p
    rinv = pow(R, -1, p)
    to_limbs = lambda v: [(v >> (30 * i)) & M30 if i < NL - 1 else v >> (30 * i) for i in range(NL)]   # noqa: E731
    from_limbs = lambda ws: sum(w << (30 * i) for i, w in enumerate(ws))                                # noqa: E731
    vals = limb_operands(p, cv.name)
    ones = R - 1
    a2 = vals + [ones, ones, 64 * p - 1]
    b2 = list(reversed(vals)) + [ones, 1, ones]
    mul = cv.ctx.test_fp_raw(_lib.OP_MUL, [to_limbs(v) for v in a2], [to_limbs(v) for v in b2])
    sqr = cv.ctx.test_fp_raw(_lib.OP_SQR, [to_limbs(v) for v in a2], [to_limbs(v) for v in a2])
    for i, (x, y) in enumerate(zip(a2, b2)):
        r = from_limbs(mul[i])
        assert all(w <= M30 for w in mul[i][: NL - 1])
        assert r % p == x * y * rinv % p and r < p + x * y // R + 1, i
        if 2 * x * y < R * p:
            assert r < p + p // 2
        r = from_limbs(sqr[i])
        assert r % p == x * x * rinv % p and r < p + x * x // R + 1, i


def test_glv_decompose(cv):
    B = cv.B
    g = O.glv_params(B.q, B.lam)
    scalars = [0, 1, 2, B.q - 1, B.q - 2, B.lam, B.lam - 1, B.lam + 1, B.q // 2] + O.prng_ints(f"gpu/cycles/glv/{cv.name}", 1 << 14, B.q)
    got = cv.ctx.test_glv(O.scalars_to_bytes(scalars))
    for s, r in zip(scalars, got):
        assert tuple(r) == O.glv_decompose(s, g), hex(s)
        assert max(r[0].bit_length(), r[1].bit_length()) <= g.max_bits


def proj_bytes(P, z, p):
    X, Y, Z = (0, z % p or 1, 0) if P is None else (P[0] * z % p, P[1] * z % p, z % p)
    return tb(X) + tb(Y) + tb(Z)


def proj_affine(b, p):
    X, Y, Z = (fb(b, i) for i in range(3))
    if Z == 0:
        return None
    zi = pow(Z, -1, p)
    return (X * zi % p, Y * zi % p)


def test_projective_curve_operators(cv):
    ctx, B, p = cv.ctx, cv.B, cv.B.p
    pts = [cv.dlog_point(k) for k in (1, 2, 3, 5, 7, 11, 1234567, B.q - 1, B.q - 2)]
    zs = O.prng_ints(f"gpu/cycles/proj/{cv.name}", 64, p - 1)
    pairs = [(P, Q) for i, P in enumerate(pts) for Q in (pts[(i + 1) % len(pts)], P, O.aff_neg(P, p), None)] + [(None, pts[0]), (None, None)]
    pb = b"".join(proj_bytes(P, zs[i % 64] + 1, p) for i, (P, _) in enumerate(pairs))
    qb = b"".join(proj_bytes(Q, zs[(i + 7) % 64] + 1, p) for i, (_, Q) in enumerate(pairs))
    pt = 3 * CB
    out = ctx.test_curve_op(0, pb, qb)
    for i, (P, Q) in enumerate(pairs):
        assert proj_affine(out[pt * i : pt * i + pt], p) == O.aff_add(P, Q, p), ("add", i)
    out = ctx.test_curve_op(1, pb, qb)
    for i, (P, _) in enumerate(pairs):
        assert proj_affine(out[pt * i : pt * i + pt], p) == (None if P is None else O.aff_double(P, p)), ("double", i)
    qa = b"".join((b"\0" * pt) if Q is None else (tb(Q[0]) + tb(Q[1]) + tb(12345)) for _, Q in pairs)
    out = ctx.test_curve_op(2, pb, qa)
    for i, (P, Q) in enumerate(pairs):
        assert proj_affine(out[pt * i : pt * i + pt], p) == O.aff_add(P, Q, p), ("mixed", i)


def pair_mix(cv, n, seed):
    """generic pairs with P + P, P - P and identity operands mixed in"""
    p = cv.B.p
    base, _ = O.random_points_bls377(f"gpu/cycles/pairs/{cv.name}/{seed}", 40, cv.B)
    g, h = [], []
    for i in range(n):
        P, Q = base[i % 40], base[(i * 11 + 5) % 40]
        k = i % 19
        if k == 3: Q = P
        elif k == 6: Q = O.aff_neg(P, p)
        elif k == 9: Q = None
        elif k == 12: P = None
        elif k == 15: P, Q = None, None
        g.append(P)
        h.append(Q)
    memo = {}
    exp = []
    for key in zip(g, h):
        if key not in memo:
            memo[key] = O.aff_add(key[0], key[1], p)
        exp.append(memo[key])
    return g, h, exp


def test_batch_add_gather(cv):
    g, h, exp = pair_mix(cv, 5003, "gather")
    out = cv.ctx.test_batch_add(b"".join(map(enc_pt, g)), b"".join(map(enc_pt, h)))
    for i, e in enumerate(exp):
        assert dec_pt(out, i) == e, i


def test_packed_chains_on_edge_operands(cv):
    """The v_subb / v_addc chains of packed.h (pk_sub, pk_add, pk_sub_mod, pk_cond_sub_p at 8 words) run in k_batch_add only.  Its
    formulas hold for any coordinates with x1 != x2 -- m = (y2 - y1) / (x2 - x1), x3 = m^2 - x1 - x2, y3 = m (x1 - x3) - y1 -- and
    msm_test_batch_add does not ask for curve points, so the operands are chosen by their STORED words (Montgomery form, v = x R):
    0, 1, p - 1, both sides of every 32-bit word boundary, so that x2 - x1, y2 - y1 and the later differences sit at 0, 1, p - 1 and
    borrow or carry across every word.  Equal x: P + P (3 x^2 / 2 y) where the y are equal and non-zero, the identity otherwise."""
    p = cv.B.p
    rinv = pow(R, -1, p)
    edge = packed_edge_values(p)
    plain = [v * rinv % p for v in edge]                 # the coordinate whose stored words are v
    rnd = O.prng_ints(f"gpu/cycles/packed/{cv.name}", 8, p)
    g, h = [], []
    for i, x1 in enumerate(plain):
        for j, x2 in enumerate(plain):
            y1, y2 = plain[(i + 3 * j + 1) % len(plain)], plain[(5 * i + j + 2) % len(plain)]
            g.append((x1, y1))
            h.append((x2, y2))
        for k, r in enumerate(rnd):                      # equal x: equal y (doubling), different y, y = 0
            y = plain[(i + k) % len(plain)]
            g.append((x1, y))
            h.append((x1, y if k % 2 == 0 else r))
    keep = [(P, Q) for P, Q in zip(g, h) if P != (0, 0) and Q != (0, 0)]      # (0, 0) is the wire's identity
    g, h = [P for P, _ in keep], [Q for _, Q in keep]

    def add(P, Q):
        (x1, y1), (x2, y2) = P, Q
        if x1 == x2:
            if y1 != y2 or y1 == 0:
                return None
            m = 3 * x1 * x1 * pow(2 * y1, -1, p) % p
        else:
            m = (y2 - y1) * pow(x2 - x1, -1, p) % p
        x3 = (m * m - x1 - x2) % p
        return x3, (m * (x1 - x3) - y1) % p

    out = cv.ctx.test_batch_add(b"".join(map(enc_pt, g)), b"".join(map(enc_pt, h)))
    assert len(g) > 900
    for i, (P, Q) in enumerate(zip(g, h)):
        e = add(P, Q)
        assert (fb(out, 2 * i), fb(out, 2 * i + 1)) == ((0, 0) if e is None else e), (i, P, Q)


@pytest.mark.parametrize("mode,steps", [(1, 1), (1, 512), (2, 2), (2, 512)])
def test_batch_add_plane_modes(cv, mode, steps):
    n = 3 * 256 * steps // 2 + 37 if steps < 512 else 512 * 256 + 11
    g, h, exp = pair_mix(cv, n, f"mode{mode}")
    out = cv.ctx.test_batch_add_mode(b"".join(map(enc_pt, g)), b"".join(map(enc_pt, h)), mode, steps)
    for i, e in enumerate(exp):
        assert dec_pt(out, i) == e, (mode, steps, i)


def test_bucket_reduce(cv):
    B, p = cv.B, cv.B.p
    K, L = 3, 64
    base, _ = O.random_points_bls377(f"gpu/cycles/reduce/{cv.name}", 24, B)
    buckets = [[None if (k * L + l) % 5 == 2 else base[(7 * k + 3 * l) % 24] for l in range(L)] for k in range(K)]
    buckets[1][5] = O.aff_neg(buckets[1][6], p) if buckets[1][6] else None
    exp = []
    for k in range(K):
        acc = None
        for l in range(L):
            if buckets[k][l] is not None:
                acc = O.aff_add(acc, O.aff_scale(l + 1, buckets[k][l], p), p)
        exp.append(acc)
    raw = b"".join(enc_pt(P) for row in buckets for P in row)

    def affine(out):
        res = []
        for k in range(K):
            X, Y, Z = (int.from_bytes(out[144 * k + 48 * j : 144 * k + 48 * j + 48], "little") for j in range(3))
            res.append(None if Z == 0 else (X * pow(Z, -1, p) % p, Y * pow(Z, -1, p) % p))
        return res

    got, ms = cv.ctx.test_bucket_reduce(raw, K, L, mode=0)
    assert affine(got) == exp
    for c0 in (0, 2, 6):
        got, _ = cv.ctx.test_bucket_reduce(raw, K, L, mode=1, c0=c0)
        assert affine(got) == exp, c0


# ---------------------------------------------------------------------------------------------- MSM parity

def test_msm_fixtures(cv):
    for c in cv.gold["msm"]:
        cv.ctx.set_points(bytes.fromhex(c["points"]), check_curve=True)
        exp = None if c["result"] is None else (int(c["result"][0], 16), int(c["result"][1], 16))
        for cc in (c["c"], None, 3, 11, 16):
            res, info = cv.ctx.run(bytes.fromhex(c["scalars"]), c=cc)
            assert res.as_tuple() == exp, (c["name"], cc, info)
        res, info = cv.ctx.run(bytes.fromhex(c["scalars"]), no_glv=True)
        assert res.as_tuple() == exp, (c["name"], "no_glv", info)


def test_msm_scalar_edges(cv):
    B, p, q = cv.B, cv.B.p, cv.B.q
    pts, _ = O.random_points_bls377(f"gpu/cycles/edge/{cv.name}", 4, B)
    for s in (1, q - 1, q - 2, B.lam, B.lam + 1, (1 << 253) + 12345, (1 << 126) - 1, 1 << 126, (1 << 127) - 1, 1 << 127, 1 << 128):
        assert run_msm(cv.ctx, [s], [pts[1]])[0] == O.aff_scale(s % q, pts[1], p), hex(s)
    assert run_msm(cv.ctx, [q + 5], [pts[2]])[0] == O.aff_scale(5, pts[2], p)
    assert run_msm(cv.ctx, [(1 << 256) - 1], [pts[2]])[0] == O.aff_scale(((1 << 256) - 1) % q, pts[2], p)
    cv.ctx.set_points(b"")
    assert cv.ctx.run(b"")[0].isZero
    info = run_msm(cv.ctx, O.prng_ints("x", 64, q), [pts[0]] * 64, 16)[1]
    assert info["K"] == -(-(CURVES[cv.name][4] + 1) // 16) == 8


@pytest.mark.parametrize("n", [256, 1000])
def test_msm_against_the_oracle_run_live(cv, n):
    """Beyond the committed fixtures (N <= 37): the Python oracle's batched-affine MSM over points generated on the GPU."""
    cv.ctx.generate_points(n, seed=900 + n)
    raw = cv.ctx.get_points(0, n)
    pts = [dec_pt(raw, i) for i in range(n)]
    sc = O.prng_ints(f"gpu/cycles/live/{cv.name}/{n}", n, cv.B.q)
    exp = O.msm_batched_affine(sc, pts, cv.B)
    for c in (None, 7):
        res, info = cv.ctx.run(O.scalars_to_bytes(sc), c=c, no_tables=True)
        assert res.as_tuple() == exp, (c, info)


@pytest.mark.parametrize("lg", [12, 14, 16])
def test_msm_known_discrete_logs(cv, lg):
    n = 1 << lg
    dev, s, exp = generated(cv, n, 300 + lg)
    res, info = cv.ctx.run_device(dev, n, no_tables=True)
    assert res.as_tuple() == exp and not info["tables"], info
    res, info = cv.ctx.run_device(dev, n)              # the default plan: window tables where the library builds them
    assert res.as_tuple() == exp, info
    for c in (8, 13):
        assert cv.ctx.run_device(dev, n, c=c, no_tables=True)[0].as_tuple() == exp, c
    assert cv.ctx.run_device(dev, n, no_glv=True, no_tables=True)[0].as_tuple() == exp


def test_msm_2p20_every_sort_path_and_tables(cv):
    """2^20 points: the one-level sort (c = 11), the radix split (16), the bin split (18: the folded top window at 126 bits, a
    short one at 127; 21), without GLV, and on window tables (default plan and an explicit precompute)."""
    n = 1 << 20
    dev, s, exp = generated(cv, n, 520)
    for c in (11, 16, 18, 21):
        res, info = cv.ctx.run_device(dev, n, c=c, no_tables=True)
        assert res.as_tuple() == exp and info["c"] == c and not info["tables"], info
    assert cv.ctx.run_device(dev, n, no_glv=True, no_tables=True)[0].as_tuple() == exp
    res, info = cv.ctx.run_device(dev, n)
    assert res.as_tuple() == exp, info
    for c in (16, 18):
        cc, K, nbytes = cv.ctx.precompute(n, c=c)
        res, info = cv.ctx.run_device(dev, n, c=c)
        assert info["tables"] and info["K"] == K and res.as_tuple() == exp, (c, info)


def test_msm_2p24(cv):
    n = 1 << 24
    dev, s, exp = generated(cv, n, 624)
    res, info = cv.ctx.run_device(dev, n, no_tables=True)
    assert res.as_tuple() == exp, info
    res, info = cv.ctx.run_device(dev, n)
    assert res.as_tuple() == exp, info
    for c in (11, 16):          # the one-level sort and the radix split (the default plan above is the bin split)
        res, info = cv.ctx.run_device(dev, n, c=c, no_tables=True)
        assert res.as_tuple() == exp and info["c"] == c, info
    assert cv.ctx.run_device(dev, n, no_glv=True, no_tables=True)[0].as_tuple() == exp


# ---------------------------------------------------------------------------------------------- inherited features

def test_run_batch_equals_run(cv):
    n = 1 << 12
    cv.ctx.generate_points(n, seed=41)
    vecs = [O.scalars_to_bytes(O.prng_ints(f"gpu/cycles/batch/{cv.name}/{b}", n, cv.B.q)) for b in range(5)]
    single = [cv.ctx.run(v, no_tables=True)[0].as_tuple() for v in vecs]
    _, one = cv.ctx.run(vecs[0], no_tables=True)
    got = cv.ctx.run_batch(vecs, no_tables=True)
    assert [r.as_tuple() for r, _ in got] == single
    # the fused path was taken: the five elements share the tree rounds (element by element every call has its own)
    assert got[0][1]["rounds"] < 5 * one["rounds"], (got[0][1], one)


def test_run_narrow_equals_run(cv):
    import numpy as np

    from montgomery_amd import MsmError
    from montgomery_amd import narrow as N

    n = 3000
    cv.ctx.generate_points(n, seed=43)
    rng = np.random.default_rng(7)
    u64 = rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)
    i32 = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
    for arr in (u64, i32):
        wide = b"".join((int(v) % cv.B.q).to_bytes(32, "little") for v in arr)
        assert cv.ctx.run_narrow(arr)[0].as_tuple() == cv.ctx.run(wide, no_tables=True)[0].as_tuple(), arr.dtype
    vals = O.prng_ints(f"gpu/cycles/narrow/{cv.name}", n, 1 << 40)
    wide = O.scalars_to_bytes(vals)
    assert cv.ctx.run_narrow(wide, bits=40, width=32)[0].as_tuple() == cv.ctx.run(wide, no_tables=True)[0].as_tuple()
    assert cv.ctx.scalar_bits(wide)[0] <= 40
    bad = bytearray(wide)
    bad[32 * 1234 + 5] |= 0x01      # bit 40 of scalar 1234
    with pytest.raises(MsmError) as e:
        cv.ctx.run_narrow(bytes(bad), bits=40, width=32)
    assert e.value.code == 6


def test_window_sums_and_combine_groups(cv):
    from montgomery_amd import distributed as D

    n = 2000
    cv.ctx.generate_points(n, seed=47)
    sb = O.scalars_to_bytes(O.prng_ints(f"gpu/cycles/shard/{cv.name}", n, cv.B.q))
    full, info = cv.ctx.run(sb, c=13, no_tables=True)
    K = info["K"]
    # two-way window split: rank r computes windows [lo, hi) over all points; the Horner step takes the K sums
    parts = cv.ctx.window_sums(sb, n, 0, K // 2, c=13)[0] + cv.ctx.window_sums(sb, n, K // 2, K, c=13)[0]
    assert cv.ctx.combine(parts, K, 13).as_tuple() == full.as_tuple()
    assert D.combine_host(parts, K, 13, cv.cid) == full.as_tuple()
    # two-way points split: group g computes all windows over its half of the points
    h = n // 2
    g0 = cv.ctx.window_sums(sb[: 32 * h], h, 0, K, c=13, point_lo=0)[0]
    g1 = cv.ctx.window_sums(sb[32 * h :], n - h, 0, K, c=13, point_lo=h)[0]
    assert D.combine_groups_host(g0 + g1, 2, K, 13, cv.cid) == full.as_tuple()


def test_windows_over_point_ranges(cv):
    """The sums of the ranges of the points a tight msm_set_workspace_limit cuts every window into, added on the host, on an
    8-word field (tests/test_gpu_boundary.py has the 12-word and the Edwards case).  A range is never shorter than 4096 points,
    so n = 2^13 + 321 is the smallest size that still splits in three; at c = 16 the bucket counters of one window alone exceed
    the boundary test's 60 MB limit.  Against the known discrete logs, through msm_run and through msm_window_sums."""
    n = (1 << 13) + 321
    dev, s, exp = generated(cv, n, 710)
    ref, info0 = cv.ctx.run_device(dev, n, c=16, no_tables=True)
    assert ref.as_tuple() == exp
    cv.ctx.set_workspace_limit(60 << 20)
    try:
        got, info1 = cv.ctx.run_device(dev, n, c=16, no_tables=True)
        assert got.as_tuple() == exp
        assert info1["rounds"] > info0["rounds"], (info0["rounds"], info1["rounds"])
        K = info0["K"]
        part, _ = cv.ctx.window_sums(dev, n, 0, K, c=16, on_device=True)
        assert cv.ctx.combine(part, K, 16).as_tuple() == exp
    finally:
        cv.ctx.set_workspace_limit(0)


def test_device_list_sums_over_the_devices(cv):
    """A device list [0, 0]: every device runs all windows over half of the points, the two sums of every window are added on the
    host (8-word field; tests/test_gpu_boundary.py has the 12-word and the Edwards case).  Several windows (c = 8), against the
    known discrete logs, through msm_run and through msm_window_sums."""
    from montgomery_amd.api import MsmContext
    from oracle import c_oracle

    n = (1 << 11) + 77
    multi = MsmContext(cv.cid, devices=[0, 0])
    try:
        a = multi.generate_points(n, seed=720, want_scalars=True)
        _, s = multi.generate_scalars(n, seed=721, to_host=True)
        exp = cv.dlog_point(c_oracle.dot_mod(a, s, n, cv.B.q))
        res, info = multi.run(s, c=8)
        assert res.as_tuple() == exp and info["K"] > 2, info
        part, _ = multi.window_sums(s, n, 0, info["K"], c=8)
        assert multi.combine(part, info["K"], 8).as_tuple() == exp
    finally:
        multi.close()


def test_skewed_scalars(cv):
    n = 1 << 18
    dev, s, exp = generated(cv, n, 718)
    a = cv.ctx.generate_points(n, seed=718, want_scalars=True, raw=True)
    from oracle import c_oracle

    one = O.prng_ints(f"gpu/cycles/skew/{cv.name}", 1, cv.B.q)[0]
    sb = one.to_bytes(32, "little") * n
    exp = cv.dlog_point(c_oracle.dot_mod(a, sb, n, cv.B.q))
    res, info = cv.ctx.run(sb, no_tables=True)
    assert res.as_tuple() == exp, info
    assert cv.ctx.run(sb)[0].as_tuple() == exp


# ---------------------------------------------------------------------------------------------- ingest

def _expect_refused(fn, index, reason):
    from montgomery_amd import MsmError

    with pytest.raises(MsmError) as e:
        fn()
    assert e.value.code == 3 and e.value.bad_index == index, str(e.value)
    assert f"point {index}: {reason}" in str(e.value), str(e.value)


def test_compressed_load_equals_uncompressed(cv):
    n = 1 << 12
    cv.ctx.generate_points(n, seed=53)
    raw = cv.ctx.get_points(0, n)
    comp = cv.ctx.get_points(0, n, compressed=True)
    pts = [dec_pt(raw, i) for i in range(n)]
    assert comp == b"".join(compress(cv.name, P) for P in pts)      # the encoder against the Python codec
    assert all(decompress(cv.name, comp[32 * i : 32 * i + 32]) == pts[i] for i in range(0, n, 97))
    for validate in ("subgroup", "none"):
        assert cv.ctx.load_points(comp, compressed=True, validate=validate) == n
        assert cv.ctx.get_points(0, n) == raw
    ident = compress(cv.name, None)
    cv.ctx.load_points(comp[:64] + ident + comp[64:128], compressed=True)
    assert cv.ctx.get_points(2, 1) == bytes(64) and cv.ctx.get_points(2, 1, compressed=True) == ident
    assert cv.ctx.load_points(raw, validate="subgroup") == n


def test_refusals_with_their_index(cv):
    B, p = cv.B, cv.B.p
    n, at = 1 << 12, 1234
    cv.ctx.generate_points(n, seed=59)
    raw = cv.ctx.get_points(0, n)
    comp = cv.ctx.get_points(0, n, compressed=True)
    plant = lambda enc: comp[: 32 * at] + enc + comp[32 * at + 32 :]   # noqa: E731
    x_none = next(x for x in range(2, 200) if O.sqrt_mod((x ** 3 + B.b) % p, p) is None)
    bad = [("coordinate >= p", tb(p)), ("coordinate >= p", tb(p + 7)), ("no curve point", tb(x_none))]
    if cv.pasta:
        bad.append(("no curve point", bytes(31) + b"\x80"))
    else:
        bad += [("invalid flags", bytes(31) + b"\xc0"), ("invalid flags", b"\x01" + bytes(30) + b"\x40")]
    for reason, enc in bad:
        assert decompress(cv.name, enc) == reason                       # the Python codec refuses it for the same reason
        _expect_refused(lambda: cv.ctx.load_points(plant(enc), compressed=True, validate="none"), at, reason)
    # the smallest bad index wins
    two = comp[: 32 * 100] + tb(p) + comp[32 * 101 : 32 * at] + tb(x_none) + comp[32 * at + 32 :]
    _expect_refused(lambda: cv.ctx.load_points(two, compressed=True), 100, "coordinate >= p")
    # uncompressed: an off-curve point under "curve", a coordinate >= p under none
    P = dec_pt(raw, at)
    off = raw[: 64 * at] + tb(P[0]) + tb((P[1] + 1) % p) + raw[64 * at + 64 :]
    _expect_refused(lambda: cv.ctx.load_points(off, validate="curve"), at, "not on curve")
    _expect_refused(lambda: cv.ctx.load_points(off, validate="subgroup"), at, "not on curve")
    assert cv.ctx.load_points(off, validate=None) == n                  # not checked: loads
    _expect_refused(lambda: cv.ctx.validate_points(level="curve"), at, "not on curve")
    big = raw[: 64 * at] + tb(P[0]) + tb(p + 1) + raw[64 * at + 64 :]
    _expect_refused(lambda: cv.ctx.load_points(big, validate=None), at, "coordinate >= p")


# ---------------------------------------------------------------------------------------------- facades

def test_python_facade_compute_msm(cv):
    from montgomery_amd import api

    params = {"bn254": api.BN254, "grumpkin": api.GRUMPKIN, "vesta": api.VESTA}[cv.name]
    B = cv.B
    assert (params.modulus, params.order, params.b % B.p, params.generator, params.endomorphism) == (B.p, B.q, B.b, (B.gx, B.gy), (B.lam, B.beta))
    pts, _ = O.random_points_bls377(f"gpu/cycles/api/{cv.name}", 50, B)
    sc = O.prng_ints(f"gpu/cycles/api/{cv.name}/s", 50, B.q)
    exp = O.msm_batched_affine(sc, pts, B)
    mod = api.Weierstrass.create(params)
    try:
        out = api.compute_msm(O.points_to_bytes(pts, 32), O.scalars_to_bytes(sc), mod)
        assert (out["x"], out["y"]) == exp
        dicts = [{"x": P[0], "y": P[1], "isZero": False} for P in pts]
        out = api.compute_msm(dicts, sc, mod)
        assert (out["x"], out["y"]) == exp
        par = mod.Parallel
        pp, sp = par.getPointer(50 * 64), par.getScalarPointer(50 * 32)
        par.pointsFromBytes(pp, O.points_to_bytes(pts, 32), 50)
        par.scalarsFromBytes(sp, O.scalars_to_bytes(sc), 50)
        assert par.msmUnsafe(sp, pp, 50, True, {"c": 6})["result"].as_tuple() == exp
    finally:
        mod.context.close()
    out = api.compute_msm(O.points_to_bytes(pts, 32), O.scalars_to_bytes(sc), params)   # parameters: a module for this call
    assert (out["x"], out["y"]) == exp


def test_js_facade():
    """js/test-cycle-curves.js: the three curves through js/montgomery-hip.js and the N-API addon."""
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    node = shutil.which("node") or shutil.which("nodejs")
    assert node, "node is part of the image the other N-API tests run on"
    from conftest import build_if_missing

    build_if_missing("napi", "montgomery_amd/msm_hip.node")
    out = subprocess.run([node, os.path.join(root, "js", "test-cycle-curves.js")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "cycle curves ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
