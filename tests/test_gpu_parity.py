"""Parity of the HIP path (through the C ABI) against the CPU oracle.  Needs an MI355X: `-m gpu`.

Structure follows the reference's own tests: backend operator vs spec (src/field.test.ts),
batch add vs single adds, MSM vs bigint MSM for N = 2^0 .. 2^12 (src/msm.test.ts:44-82), plus the
fixed-point known-answer scripts (scripts/zprize23/submission-test-bls377.ts).  Everything is
bit-exact: canonical affine (x, y) or the identity.
"""
import json
import os

import pytest

from oracle import msm_oracle as O

pytestmark = pytest.mark.gpu

C = O.BLS12_377
P_MOD = C.p
R = 1 << 390
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def H(x):
    return int(x, 16)


def tb(v):
    return v.to_bytes(48, "little")


def fb(b, i):
    return int.from_bytes(b[48 * i : 48 * i + 48], "little")


def enc_pt(P):
    return b"\0" * 96 if P is None else tb(P[0]) + tb(P[1])


def run_msm(ctx, scalars, points, c=None):
    ctx.set_points(b"".join(enc_pt(P) for P in points), check_curve=True)
    res, info = ctx.run(O.scalars_to_bytes(scalars), c=c)
    return res.as_tuple(), info


# ---- the library that ran is the in-tree HIP extension ------------------------------------------


def test_native_library_is_loaded(gpu_ctx):
    from montgomery_amd import _lib

    maps = open("/proc/self/maps").read()
    assert os.path.realpath(_lib.LIB_PATH) in maps


# ---- field operators (src/field.test.ts:27-155) --------------------------------------------------


def field_inputs():
    p = P_MOD
    special = [0, 1, 2, p - 1, p - 2, (p + 1) // 2, 1 << 376, (1 << 30) - 1, 1 << 30, (1 << 360) + 5]
    return special + O.prng_ints("gpu/fp", 500, p)


def test_fp_mul_sqr_add_sub(gpu_ctx):
    from montgomery_amd import _lib

    vals = field_inputs()
    n = len(vals)
    a = b"".join(tb(v) for v in vals)
    b = b"".join(tb(v) for v in reversed(vals))
    rinv = pow(R, -1, P_MOD)
    out = gpu_ctx.test_fp(_lib.OP_MUL, a, b)
    assert all(fb(out, i) == vals[i] * vals[n - 1 - i] * rinv % P_MOD for i in range(n))
    out = gpu_ctx.test_fp(_lib.OP_SQR, a)
    assert all(fb(out, i) == vals[i] * vals[i] * rinv % P_MOD for i in range(n))
    out = gpu_ctx.test_fp(_lib.OP_ADD, a, b)
    assert all(fb(out, i) == (vals[i] + vals[n - 1 - i]) % P_MOD for i in range(n))
    out = gpu_ctx.test_fp(_lib.OP_SUB, a, b)
    assert all(fb(out, i) == (vals[i] - vals[n - 1 - i]) % P_MOD for i in range(n))


def test_fp_montgomery_roundtrip_and_inverse(gpu_ctx):
    from montgomery_amd import _lib

    vals = [v for v in field_inputs() if v]
    a = b"".join(tb(v) for v in vals)
    mont = gpu_ctx.test_fp(_lib.OP_TO_MONT, a)
    assert all(fb(mont, i) == v * R % P_MOD for i, v in enumerate(vals))
    assert gpu_ctx.test_fp(_lib.OP_FROM_MONT, mont) == a
    inv = gpu_ctx.test_fp(_lib.OP_INV, mont)            # (a R)^-1 R^2 = a^-1 R
    back = gpu_ctx.test_fp(_lib.OP_FROM_MONT, inv)
    assert all(fb(back, i) == pow(v, -1, P_MOD) for i, v in enumerate(vals))


def test_fp_inverse_variants_agree(gpu_ctx):
    """division steps (the product's `fe_inv`), Fermat, and Kaliski's almost-inverse -- the reference's
    own algorithm, src/wasm/inverse.ts:136-218 -- give the same Montgomery-form inverse on the GPU."""
    from montgomery_amd import _lib

    vals = [v for v in field_inputs() if v][:300]
    mont = gpu_ctx.test_fp(_lib.OP_TO_MONT, b"".join(tb(v) for v in vals))
    ref = gpu_ctx.test_fp(_lib.OP_INV, mont)
    assert gpu_ctx.test_fp(_lib.OP_INV_FERMAT, mont) == ref
    assert gpu_ctx.test_fp(_lib.OP_INV_KALISKI, mont) == ref
    # fourth variant: the reference's experimental word-sliced almost-inverse, src/inverse/faster-inverse-wasm.ts:133-343
    assert gpu_ctx.test_fp(_lib.OP_INV_WORDSLICED, mont) == ref
    back = gpu_ctx.test_fp(_lib.OP_FROM_MONT, ref)
    assert all(fb(back, i) == pow(v, -1, P_MOD) for i, v in enumerate(vals))


def test_fp_golden(gpu_ctx):
    from montgomery_amd import _lib

    cases = load("fp377.json")["cases"]
    a = b"".join(tb(H(c["a"])) for c in cases)
    b = b"".join(tb(H(c["b"])) for c in cases)
    am, bm = gpu_ctx.test_fp(_lib.OP_TO_MONT, a), gpu_ctx.test_fp(_lib.OP_TO_MONT, b)
    for op, key in ((_lib.OP_MUL, "mul"), (_lib.OP_ADD, "add"), (_lib.OP_SUB, "sub"), (_lib.OP_SQR, "sqr")):
        out = gpu_ctx.test_fp(_lib.OP_FROM_MONT, gpu_ctx.test_fp(op, am, bm))
        assert [fb(out, i) for i in range(len(cases))] == [H(c[key]) for c in cases], key


def test_batch_inverse(gpu_ctx):
    """`batchInverse` vs single inverses for several batch lengths (src/field.test.ts:152-211)."""
    from montgomery_amd import _lib

    vals = [v for v in field_inputs() if v][:203]
    mont = gpu_ctx.test_fp(_lib.OP_TO_MONT, b"".join(tb(v) for v in vals))
    for per_lane in (1, 2, 7, 100, 1000):
        out = gpu_ctx.test_fp(_lib.OP_FROM_MONT, gpu_ctx.test_batch_inverse(mont, per_lane))
        assert all(fb(out, i) == pow(v, -1, P_MOD) for i, v in enumerate(vals)), per_lane


# ---- GLV decomposition (src/glv/glv-test.ts:92-125) ------------------------------------------------


def test_glv_decompose(gpu_ctx, c_oracle):
    g = O.glv_params(C.q, C.lam)
    scalars = [H(c["s"]) for c in load("glv377.json")["cases"]] + O.prng_ints("gpu/glv", 20000, C.q)
    got = gpu_ctx.test_glv(O.scalars_to_bytes(scalars))
    for s, r in zip(scalars[:3000], got):
        assert tuple(r) == O.glv_decompose(s, g)
    for s, r in zip(scalars[3000:], got[3000:]):
        assert tuple(r) == c_oracle.glv_decompose(s)


# ---- batched affine addition (src/curve-affine.ts:376-522) -----------------------------------------


def test_batch_add_golden_and_random(gpu_ctx):
    dec = lambda P: None if P is None else (H(P[0]), H(P[1]))
    cases = load("point_add377.json")["cases"]
    gs = [dec(c["g"]) for c in cases]
    hs = [dec(c["h"]) for c in cases]
    exp = [dec(c["sum"]) for c in cases]
    pts, _ = O.random_points_bls377("gpu/batch", 600)
    gs += pts[:300]
    hs += pts[300:]
    exp += [O.aff_add(a, b, P_MOD) for a, b in zip(pts[:300], pts[300:])]
    out = gpu_ctx.test_batch_add(b"".join(map(enc_pt, gs)), b"".join(map(enc_pt, hs)))
    for i, e in enumerate(exp):
        got = (fb(out, 2 * i), fb(out, 2 * i + 1))
        assert got == ((0, 0) if e is None else e), i


# ---- MSM vs oracle --------------------------------------------------------------------------------


def test_msm_golden_vectors(gpu_ctx):
    for c in load("msm377.json")["cases"]:
        gpu_ctx.set_points(bytes.fromhex(c["points"]))
        exp = None if c["result"] is None else (H(c["result"][0]), H(c["result"][1]))
        for cc in (c["c"], None, 3, 11):
            res, info = gpu_ctx.run(bytes.fromhex(c["scalars"]), c=cc)
            assert res.as_tuple() == exp, (c["name"], cc, info)


def test_msm_sizes_like_reference_msm_test(gpu_ctx, c_oracle):
    """N = 2^0, 2^2, ..., 2^12 (src/msm.test.ts:44-82): GPU == C oracle == known-discrete-log answer."""
    pts, ks = O.random_points_bls377("gpu/sizes", 4096)
    G = (C.gx, C.gy)
    for lg in range(0, 13, 2):
        n = 1 << lg
        sc = O.prng_ints(f"gpu/sizes/{lg}", n, C.q)
        got, info = run_msm(gpu_ctx, sc, pts[:n])
        exp = O.aff_scale(sum(a * b for a, b in zip(sc, ks[:n])) % C.q, G, P_MOD)
        assert got == exp, (lg, info)
        ref, _ = c_oracle.msm_bls377(O.points_to_bytes(pts[:n], 48), O.scalars_to_bytes(sc), 0)
        assert ref == exp


def test_msm_ragged_sizes_and_windows(gpu_ctx, c_oracle):
    pts, _ = O.random_points_bls377("gpu/ragged", 777)
    for n, c in ((1, 2), (2, 16), (3, 5), (17, 9), (100, 13), (255, 6), (777, 8), (777, 10), (513, 12)):
        sc = O.prng_ints(f"gpu/ragged/{n}/{c}", n, C.q)
        got, info = run_msm(gpu_ctx, sc, pts[:n], c)
        ref, _ = c_oracle.msm_bls377(O.points_to_bytes(pts[:n], 48), O.scalars_to_bytes(sc), 0)
        assert got == ref, (n, c, info)
        assert info["c"] == c


def test_msm_edge_cases(gpu_ctx):
    pts, _ = O.random_points_bls377("gpu/edge", 64)
    P = O.ZPRIZE_BLS377_POINT
    q = C.q
    # empty input
    gpu_ctx.set_points(b"")
    res, _ = gpu_ctx.run(b"")
    assert res.isZero
    # reference fixed-point KATs
    assert run_msm(gpu_ctx, [2, q - 1], [P, P])[0] == P
    sc = O.prng_ints("gpu/edge/same", 1000, q)
    assert run_msm(gpu_ctx, sc, [P] * 1000)[0] == run_msm(gpu_ctx, [sum(sc) % q], [P])[0]
    # all scalars zero / cancellation -> identity
    assert run_msm(gpu_ctx, [0] * 10, pts[:10])[0] is None
    assert run_msm(gpu_ctx, [5, q - 5], [pts[0], pts[0]])[0] is None
    assert run_msm(gpu_ctx, [9, 9], [pts[0], O.aff_neg(pts[0], P_MOD)])[0] is None
    # scalar extremes
    for s in (1, q - 1, q - 2, C.lam, (1 << 252) + 12345, (1 << 126) - 1, 1 << 126):
        assert run_msm(gpu_ctx, [s], [pts[1]])[0] == O.aff_scale(s, pts[1], P_MOD), hex(s)
    # scalars >= q are reduced
    assert run_msm(gpu_ctx, [q + 5], [pts[2]])[0] == O.aff_scale(5, pts[2], P_MOD)
    assert run_msm(gpu_ctx, [(1 << 256) - 1], [pts[2]])[0] == O.aff_scale(((1 << 256) - 1) % q, pts[2], P_MOD)
    # identity among the inputs, repeated points, P and -P in one bucket
    sc = O.prng_ints("gpu/edge/mix", 48, q)
    mix = list(pts[:48])
    mix[3] = None
    mix[5] = mix[4]; sc[5] = sc[4]
    mix[7] = O.aff_neg(mix[6], P_MOD); sc[7] = sc[6]
    for c in (4, 7, None):
        assert run_msm(gpu_ctx, sc, mix, c)[0] == O.msm_batched_affine(sc, mix, c=6), c
    # fewer scalars than resident points uses the first n points
    gpu_ctx.set_points(b"".join(enc_pt(Q) for Q in pts))
    sc = O.prng_ints("gpu/edge/prefix", 20, q)
    res, _ = gpu_ctx.run(O.scalars_to_bytes(sc))
    assert res.as_tuple() == O.msm_batched_affine(sc, pts[:20], c=5)


def test_msm_error_codes(gpu_ctx):
    from montgomery_amd import MsmError

    pts, _ = O.random_points_bls377("gpu/err", 4)
    with pytest.raises(MsmError) as e:
        gpu_ctx.set_points(tb(P_MOD) + tb(1))             # coordinate >= p
    assert e.value.code == 3
    with pytest.raises(MsmError) as e:
        gpu_ctx.set_points(tb(5) + tb(7), check_curve=True)  # not on the curve
    assert e.value.code == 3
    gpu_ctx.set_points(b"".join(enc_pt(Q) for Q in pts))
    with pytest.raises(MsmError) as e:
        gpu_ctx.run(O.scalars_to_bytes([1] * 5))            # more scalars than points
    assert e.value.code == 4
    with pytest.raises(MsmError) as e:
        gpu_ctx.run(O.scalars_to_bytes([1]), c=40)          # bad window size
    assert e.value.code == 1


def test_window_shards_combine_to_full_msm(gpu_ctx):
    """The multi-GPU decomposition on one GPU: P_k shards -> msm_combine == msm_run."""
    n = 300
    pts, _ = O.random_points_bls377("gpu/shard", n)
    sc = O.prng_ints("gpu/shard/s", n, C.q)
    full, info = run_msm(gpu_ctx, sc, pts, 8)
    K = info["K"]
    sb = O.scalars_to_bytes(sc)
    parts = b""
    for lo in range(0, K, 3):
        pb, _ = gpu_ctx.window_sums(sb, n, lo, min(K, lo + 3), c=8)
        parts += pb
    assert gpu_ctx.combine(parts, K, 8).as_tuple() == full
    # each shard agrees with the oracle's partition sum as a group element
    g = O.glv_params(C.q, C.lam)
    for k in range(K):
        X, Y, Z = (int.from_bytes(parts[144 * k + 48 * j : 144 * k + 48 * j + 48], "little") for j in range(3))
        got = O.proj_to_affine((X, Y, Z), P_MOD)
        exp = None
        for s, Pt in zip(sc, pts):
            a0, a1, n0, n1 = O.glv_decompose(s, g)
            for a, neg, Q in ((a0, n0, Pt), (a1, n1, (C.beta * Pt[0] % P_MOD, Pt[1]))):
                l, dneg = O.signed_digits(a, 8, K)[k]
                if l:
                    T = O.aff_scale(l, Q, P_MOD)
                    exp = O.aff_add(exp, O.aff_neg(T, P_MOD) if neg ^ dneg else T, P_MOD)
        assert got == exp, k


# ---- large sizes: size-independent properties --------------------------------------------------------


def test_generated_points_are_valid_and_known(gpu_ctx):
    n = 2000
    a = O.scalars_from_bytes(gpu_ctx.generate_points(n, seed=11, want_scalars=True))
    G = (C.gx, C.gy)
    for i in (0, 1, 2, 999, 1999):
        assert gpu_ctx.get_point(i) == O.aff_scale(a[i], G, P_MOD)
    dev, sb = gpu_ctx.generate_scalars(n, seed=5, to_host=True)
    s = O.scalars_from_bytes(sb)
    assert all(v < C.q for v in s) and len(set(s)) == n
    res, _ = gpu_ctx.run_device(dev, n)
    assert res.as_tuple() == O.aff_scale(sum(x * y for x, y in zip(a, s)) % C.q, G, P_MOD)


@pytest.mark.parametrize("lg", [16, 20])
def test_msm_large_known_discrete_logs(gpu_ctx, lg):
    """sum s_i P_i = (sum s_i a_i) G with P_i = a_i G generated on the GPU (BASELINE configs[1] = 2^20)."""
    n = 1 << lg
    a = O.scalars_from_bytes(gpu_ctx.generate_points(n, seed=100 + lg, want_scalars=True))
    dev, sb = gpu_ctx.generate_scalars(n, seed=200 + lg, to_host=True)
    s = O.scalars_from_bytes(sb)
    res, info = gpu_ctx.run_device(dev, n)
    G = (C.gx, C.gy)
    assert res.as_tuple() == O.aff_scale(sum(x * y for x, y in zip(a, s)) % C.q, G, P_MOD), info
    # independence of the window size (the result is a group element, not a function of c)
    res2, _ = gpu_ctx.run_device(dev, n, c=11)
    assert res2.as_tuple() == res.as_tuple()


def test_msm_2p26_known_discrete_logs(gpu_ctx, c_oracle):
    """BASELINE configs[2], the size the headline number is quoted on: 2^26 distinct points P_i = a_i G, 2^26 uniform
    scalars, sum s_i P_i == (sum s_i a_i mod q) G.  The dot product runs in the C oracle (OpenMP); the reference checks
    every size it benchmarks the same way against its slow path (src/msm.test.ts:64-70, scripts/msm-weierstrass.ts:97-107)."""
    n = 1 << 26
    a = gpu_ctx.generate_points(n, seed=2626, want_scalars=True, raw=True)
    dev, s = gpu_ctx.generate_scalars(n, seed=6262, to_host=True, raw=True)
    res, info = gpu_ctx.run_device(dev, n)
    k = c_oracle.dot_mod(a, s, n, C.q)
    # the generated points themselves against the oracle: 1 024 of them spread over the whole table (a prime stride), so the
    # known-discrete-log check below does not rest on the generator kernels it shares its field arithmetic with
    G = (C.gx, C.gy)
    for j in range(1024):
        i = (j * 65537 * 1021 + 12345) % n
        assert gpu_ctx.get_point(i) == O.aff_scale(int.from_bytes(a[32 * i:32 * i + 32], "little"), G, P_MOD), i
    del a, s
    assert info["c"] == 21 and info["K"] == 6      # since round 4: six windows of 21 bits, the carry bit folded into the top one
    assert res.as_tuple() == O.aff_scale(k, (C.gx, C.gy), P_MOD), info
    # the pair additions the bucket sums need: one per entry (2 N K, minus the ~2^-20 zero digits) less one per non-empty
    # bucket (2^20 in each of the five lower windows, up to 2^21 in the top one); the tree issues a few per cent more
    assert 2 * n * 6 * (1 - 2 ** -18) - 7 * (1 << 20) <= info["n_pairs_algo"] <= 2 * n * 6 - 5 * (1 << 20)
    assert info["n_pairs_algo"] < info["n_pairs"] < 1.10 * info["n_pairs_algo"]
    res22, info22 = gpu_ctx.run_device(dev, n, c=22)          # the plain six-window plan
    assert res22.as_tuple() == res.as_tuple() and info22["K"] == 6
    # the round-3 window gives the same element; its pair count is the one BASELINE's K = 8 figures are quoted on
    res16, info16 = gpu_ctx.run_device(dev, n, c=16)
    assert res16.as_tuple() == res.as_tuple() and info16["K"] == 8
    assert 2 * n * 8 * (1 - 2 ** -15) - 8 * (1 << 15) <= info16["n_pairs_algo"] <= 2 * n * 8 - 7 * (1 << 15)
    # BASELINE configs[4], per-rank workload: eight one-window shards at the FULL size (what each of 8 GPUs runs under
    # `--split windows`, where K = 8 is kept so that every rank has a window), and eight points shards (`--split points`),
    # each combined as rank 0 combines them
    from montgomery_amd import _lib
    from montgomery_amd.distributed import combine_groups_host, combine_host

    parts = b"".join(gpu_ctx.window_sums(dev, n, kk, kk + 1, c=16, on_device=True)[0] for kk in range(8))
    assert combine_host(parts, 8, 16, _lib.CURVE_BLS12_377_G1) == res.as_tuple()
    share = n // 8
    cs, Ks = gpu_ctx.plan(share, no_tables=True)   # the plan the library picks for a rank's share (seven folded 18-bit windows)
    assert (cs, Ks) == (18, 7)
    groups = b"".join(gpu_ctx.window_sums(dev + 32 * g * share, share, 0, Ks, on_device=True, point_lo=g * share)[0] for g in range(8))
    assert combine_groups_host(groups, 8, Ks, cs, _lib.CURVE_BLS12_377_G1) == res.as_tuple()
    # the same eight shards each on the window tables of ITS range of the points (round 6: 7 tables x 2^23 rows = 15 GB per rank),
    # as the ranks of `--split points` run them from their second step on
    assert gpu_ctx.plan(share, merged=True, point_lo=share) == (cs, Ks)
    groups = b""
    for g in range(8):
        assert gpu_ctx.precompute(share, c=cs, point_lo=g * share)[:2] == (cs, Ks) and gpu_ctx.tables_range() == (g * share, share)
        part, pinfo = gpu_ctx.window_sums(dev + 32 * g * share, share, 0, Ks, c=cs, on_device=True, point_lo=g * share, merged=True)
        assert pinfo["tables"], pinfo
        groups += part
    assert combine_groups_host(groups, 8, Ks, cs, _lib.CURVE_BLS12_377_G1) == res.as_tuple()
    gpu_ctx.precompute(4096, point_lo=0)   # (tables of a tiny range from here on; the 15 GB buffer goes back with the next point set)
    # and eight bucket-range shards (`--split buckets`): the single-GPU plan, every rank an eighth of every window's buckets
    groups = b"".join(gpu_ctx.window_sums(dev, n, 0, 6, on_device=True, bucket_shard=(g, 8))[0] for g in range(8))
    assert combine_groups_host(groups, 8, 6, 21, _lib.CURVE_BLS12_377_G1) == res.as_tuple()


def test_default_plan_at_2p22_is_seven_folded_18_bit_windows(gpu_ctx, c_oracle):
    """2^22 <= n < 2^24 picks seven 18-bit windows with the carry bit folded into the top one (pick_window): the plan must be
    the one the library PICKS here, not only one a test forces; same element as the 16-bit plan and as the known discrete logs."""
    n = 1 << 22
    assert gpu_ctx.plan(n) == (18, 7) and gpu_ctx.plan((1 << 24) - 1) == (18, 7) and gpu_ctx.plan(1 << 24) == (21, 6) and gpu_ctx.plan((1 << 22) - 1) == (16, 8)
    a = gpu_ctx.generate_points(n, seed=2222, want_scalars=True, raw=True)
    dev, s = gpu_ctx.generate_scalars(n, seed=4444, to_host=True, raw=True)
    res, info = gpu_ctx.run_device(dev, n)
    assert info["c"] == 18 and info["K"] == 7, info
    assert res.as_tuple() == O.aff_scale(c_oracle.dot_mod(a, s, n, C.q), (C.gx, C.gy), P_MOD), info
    res16, info16 = gpu_ctx.run_device(dev, n, c=16)
    assert info16["K"] == 8 and res16.as_tuple() == res.as_tuple()


def test_glv_halves_stay_below_the_bound_a_folded_plan_relies_on(gpu_ctx):
    """Plan::fold leaves the top window unrecoded: its digit stays inside the window's 2^c buckets only while both GLV halves
    are below 2^126 (BLS12-377: Scalar.maxBits, src/wasm/glv.ts:216-226).  Extreme and random scalars through k_test_glv."""
    extremes = [0, 1, 2, C.q - 1, C.q - 2, C.q // 2, C.q // 2 + 1, C.lam, C.lam - 1, C.lam + 1, C.q - C.lam, (1 << 252) - 1, (1 << 251),
                (C.q - 1) // 3, 2 * (C.q - 1) // 3]
    scalars = [v % C.q for v in extremes] + O.prng_ints("gpu/glv/bound", 50000, C.q)
    for (s0, s1, _n0, _n1) in gpu_ctx.test_glv(O.scalars_to_bytes(scalars)):
        assert s0 < (1 << 126) and s1 < (1 << 126)


@pytest.mark.parametrize("lg,c", [(12, None), (16, None), (18, 21), (20, 18), (22, None)])
def test_bucket_range_shards(gpu_ctx, lg, c):
    """msm_opts.bucket_shard: G shards, each all windows over all points but 1 / G of every window's buckets, add up per window
    (msm_combine_groups) to the whole MSM -- G = 2, 3 (uneven ranges) and 8, plain and folded plans, every sort path."""
    from montgomery_amd import _lib
    from montgomery_amd.distributed import combine_groups_host

    n = 1 << lg
    gpu_ctx.generate_points(n, seed=900 + lg)
    dev, _ = gpu_ctx.generate_scalars(n, seed=901 + lg)
    cc, K = gpu_ctx.plan(n, c, no_tables=True)
    want, _ = gpu_ctx.run_device(dev, n, c=cc, no_tables=True)
    for G in (2, 3, 8):
        parts = b"".join(gpu_ctx.window_sums(dev, n, 0, K, c=cc, on_device=True, bucket_shard=(g, G))[0] for g in range(G))
        assert combine_groups_host(parts, G, K, cc, _lib.CURVE_BLS12_377_G1) == want.as_tuple(), (lg, cc, G)


def test_msm_large_linearity(gpu_ctx):
    """MSM(s) + MSM(t) = MSM(s + t) and MSM(q - s) = -MSM(s) at 2^18, host scalars (PCIe path)."""
    n = 1 << 18
    gpu_ctx.generate_points(n, seed=31)
    _, sb = gpu_ctx.generate_scalars(n, seed=32, to_host=True)
    _, tb_ = gpu_ctx.generate_scalars(n, seed=33, to_host=True)
    s, t = O.scalars_from_bytes(sb), O.scalars_from_bytes(tb_)
    rs, _ = gpu_ctx.run(sb)
    rt, _ = gpu_ctx.run(tb_)
    rst, _ = gpu_ctx.run(O.scalars_to_bytes([(x + y) % C.q for x, y in zip(s, t)]))
    assert O.aff_add(rs.as_tuple(), rt.as_tuple(), P_MOD) == rst.as_tuple()
    rneg, _ = gpu_ctx.run(O.scalars_to_bytes([(C.q - x) % C.q for x in s]))
    assert rneg.as_tuple() == O.aff_neg(rs.as_tuple(), P_MOD)


def test_reference_shaped_api(gpu_ctx):
    """`Weierstraß.create(...).Parallel.msm` / `compute_msm` facade (src/parallel.ts, submission-bls377.ts)."""
    from montgomery_amd import startThreads, stopThreads
    from montgomery_amd.api import BLS12_377_PARAMS, Weierstrass, compute_msm

    startThreads(16)   # the reference's callers bracket their MSMs with these (scripts/msm-weierstrass.ts:14,50): no-ops here
    cv = Weierstrass.create(BLS12_377_PARAMS)
    pts, _ = O.random_points_bls377("gpu/api", 50)
    sc = O.prng_ints("gpu/api/s", 50, C.q)
    par = cv.Parallel
    pp, sp = par.getPointer(50 * 96), par.getScalarPointer(50 * 32)
    par.pointsFromBytes(pp, O.points_to_bytes(pts, 48), 50)
    par.scalarsFromBytes(sp, O.scalars_to_bytes(sc), 50)
    out = par.msmUnsafe(sp, pp, 50, True, {"c": 6})
    exp = O.msm_batched_affine(sc, pts, c=6)
    assert out["result"].as_tuple() == exp and out["log"]
    # {result, log} with the reference's log shape (src/msm-common.ts:176-214): parameters, "label... x.xms" lines, total last
    import re

    log = out["log"]
    assert log[0][0]["c"] == 6 and log[0][0]["K"] == -(-127 // 6) and len(log) >= 7
    assert all(re.fullmatch(r"[a-z &()]+\.\.\. \d+\.\dms", l[0]) for l in log[1:]) and log[-1][0].startswith("msm total... ")
    assert par.msm(sp, pp, 50)["log"] == []
    # the reference's own way from `result` to bigints (scripts/msm-weierstrass.ts:89-91)
    scratch, sAffinePtr = cv.Field.getPointers(20), cv.Field.getPointer(cv.Affine.size)
    cv.Projective.toAffine(scratch, sAffinePtr, out["result"])
    s = cv.Affine.toBigint(sAffinePtr)
    assert (s["x"], s["y"]) == exp and s["isZero"] is False
    r = compute_msm([{"x": x, "y": y, "isZero": False} for x, y in pts], sc, curve=cv)
    assert (r["x"], r["y"]) == exp
    P = O.ZPRIZE_BLS377_POINT
    r = compute_msm(O.points_to_bytes([P, P], 48), O.scalars_to_bytes([2, C.q - 1]), curve=cv)
    assert (r["x"], r["y"]) == P
    # `let [pointPtr] = await Parallel.randomPointsFast(N)` (scripts/msm-weierstrass.ts:18,21): handles unpack to themselves
    [rp] = par.randomPointsFast(300, seed=3)
    [rs] = par.randomScalars(300, seed=4)
    assert par.msmUnsafe(rs, rp, 300)["result"].as_tuple() == par.msmProjective(rs, rp, 300)["result"].as_tuple() is not None
    cv.context.close()
    stopThreads()


def test_config1_inputs_2p14_on_gpu(gpu_ctx):
    """The 2^14 plumbing configuration (BASELINE configs[0]) through the GPU path: same inputs as
    tests/test_oracle_kat.py::test_config1_msm_basic_2p14_cpu_plumbing, same answer."""
    base, ks = O.random_points_bls377("cfg1", 256)
    n = 1 << 14
    sc = O.prng_ints("cfg1/s", n, C.q)
    gpu_ctx.set_points(O.points_to_bytes(base, 48) * (n // 256))
    res, info = gpu_ctx.run(O.scalars_to_bytes(sc))
    G = (C.gx, C.gy)
    assert res.as_tuple() == O.aff_scale(sum(s * ks[i & 255] for i, s in enumerate(sc)) % C.q, G, P_MOD), info


def test_large_windows_three_pass_sort(gpu_ctx):
    """Window sizes whose counters do not fit the LDS: c = 17..24 take the three-pass split (coarse / mid / fine bins, short
    top windows cut on their effective bits); every path must give the same group element (known discrete logs at 2^16)."""
    n = 1 << 16
    a = O.scalars_from_bytes(gpu_ctx.generate_points(n, seed=41, want_scalars=True))
    dev, sb = gpu_ctx.generate_scalars(n, seed=42, to_host=True)
    s = O.scalars_from_bytes(sb)
    G = (C.gx, C.gy)
    exp = O.aff_scale(sum(x * y for x, y in zip(a, s)) % C.q, G, P_MOD)
    for c in (16, 17, 18, 19, 20, 21, 22, 23, 24):   # top windows of 15, 8, 1, 13, 7, 1, 17, 12 and 7 bits
        res, info = gpu_ctx.run_device(dev, n, c=c)
        assert res.as_tuple() == exp, (c, info)
        # a top window that would hold the carry bit alone (127 = 7 * 18 + 1 = 6 * 21 + 1) is folded into the window below it:
        # one window less than the reference's ceil((b + 1) / c), the top one c + 1 bits wide
        assert info["c"] == c and info["K"] == -(-127 // c) - (1 if c in (18, 21) else 0)
    # serialised window groups (used for exclusive roofline timing) give the same answer
    res, _ = gpu_ctx.run_device(dev, n, serial=True)
    assert res.as_tuple() == exp


@pytest.mark.parametrize("c", [19, 20, 22])
def test_big_windows_chunk_ordered_round1(gpu_ctx, c_oracle, c):
    """2^23 + 4096 points (more than the 2^23 rows, 2 GB, from which round 1 may take the pair form) with windows of 2^18 .. 2^21
    buckets: the three-pass split at size.  c = 19 and c = 20 (mean bucket 64 and 32: logG >= 2) take the pair form -- round 1
    walks the tile-ordered pairs of k_bin_pairs and leaves element records, round 2 reads them back --, c = 22 (mean bucket 8)
    the slot form; asserted from the library's report.  The result must be the group element of the known discrete logs,
    whatever the window size."""
    n = (1 << 23) + 4096
    a = gpu_ctx.generate_points(n, seed=2323 + c, want_scalars=True, raw=True)
    dev, s = gpu_ctx.generate_scalars(n, seed=3232 + c, to_host=True, raw=True)
    res, info = gpu_ctx.run_device(dev, n, c=c)
    assert set(gpu_ctx.test_last_sort_paths()) == {"slots" if c == 22 else "pairs"}, (gpu_ctx.test_last_sort_paths(), info)
    k = c_oracle.dot_mod(a, s, n, C.q)
    assert info["c"] == c
    assert res.as_tuple() == O.aff_scale(k, (C.gx, C.gy), P_MOD), info
    res16, _ = gpu_ctx.run_device(dev, n)
    assert res16.as_tuple() == res.as_tuple()
    if c == 20:   # msmProjective's window structure (whole 253-bit scalars, no endomorphism: K = 13) through the same path
        resp, infop = gpu_ctx.run_device(dev, n, c=c, no_glv=True)
        assert set(gpu_ctx.test_last_sort_paths()) == {"pairs"}
        assert infop["K"] == 13 and resp.as_tuple() == res.as_tuple()


def test_skewed_buckets_tail_rounds(gpu_ctx, c_oracle):
    """Heavily skewed digit distributions (few distinct scalars, tiny scalars) force deep trees, tail rounds with
    operand descriptors and the finish kernel on very uneven buckets."""
    pts, _ = O.random_points_bls377("gpu/skew", 512)
    n = 4096
    P = [pts[i % 512] for i in range(n)]
    pb = O.points_to_bytes(P, 48)
    for name, sc in (
        ("two_values", [(12345 if i % 3 else C.q - 77) for i in range(n)]),
        ("tiny", [i % 7 for i in range(n)]),
        ("one_hot_window", [(i % 5 + 1) << 48 for i in range(n)]),
    ):
        sb = O.scalars_to_bytes(sc)
        ref, _ = c_oracle.msm_bls377(pb, sb, 0)
        gpu_ctx.set_points(pb)
        for c in (None, 5, 16):
            res, info = gpu_ctx.run(sb, c=c)
            assert res.as_tuple() == ref, (name, c, info)


def test_msm_projective_window_structure(gpu_ctx):
    """`msmProjective` (src/parallel.ts:69-87, src/msm-basic.ts:45-164): windows of the whole 253-bit scalar, no GLV.
    BASELINE configs[0] shape: N = 2^14, c = 13 -> K = ceil(254 / 13) = 20."""
    pts, ks = O.random_points_bls377("gpu/proj", 256)
    G = (C.gx, C.gy)
    for n, c, K in ((1, 13, 20), (50, 6, 43), (1 << 14, 13, 20), (1 << 14, None, None), (777, 19, 14)):
        sc = O.prng_ints(f"gpu/proj/{n}/{c}", n, C.q)
        gpu_ctx.set_points(O.points_to_bytes([pts[i & 255] for i in range(n)], 48))
        res, info = gpu_ctx.run(O.scalars_to_bytes(sc), c=c, no_glv=True)
        assert info["K"] == (K or -(-254 // info["c"])), info
        assert res.as_tuple() == O.aff_scale(sum(s * ks[i & 255] for i, s in enumerate(sc)) % C.q, G, P_MOD), (n, c, info)
        if n <= 50:
            assert res.as_tuple() == O.msm_basic_projective(sc, [pts[i & 255] for i in range(n)], C, c=c)
    # extremes: q - 1 uses the top window, scalars >= q are reduced first
    for s in (C.q - 1, C.q + 7, (1 << 253) - 1, 1 << 252):
        gpu_ctx.set_points(enc_pt(pts[3]))
        res, _ = gpu_ctx.run(O.scalars_to_bytes([s % (1 << 256)]), c=9, no_glv=True)
        assert res.as_tuple() == O.aff_scale(s % C.q, pts[3], P_MOD), hex(s)
    from montgomery_amd import MsmError

    with pytest.raises(MsmError):
        gpu_ctx.run(O.scalars_to_bytes([1]), c=3, no_glv=True)


def test_projective_windows_above_16_per_group(gpu_ctx):
    """msmProjective with a small explicit window over 2^21 points: K = ceil(254 / 13) = 20 windows in ONE window group whose
    sort is the radix split -- its window table has 16 entries, so the group is cut at 16 windows (it used to fail with
    MSM_ERR_INTERNAL).  Same group element as the default plan."""
    n = 1 << 21
    gpu_ctx.generate_points(n, seed=2113)
    dev, _ = gpu_ctx.generate_scalars(n, seed=2114)
    want, _ = gpu_ctx.run_device(dev, n)
    for c in (13, 9):
        got, info = gpu_ctx.run_device(dev, n, c=c, no_glv=True)
        assert info["K"] == -(-254 // c) and got.as_tuple() == want.as_tuple(), info


def test_single_window_shards_split_by_points(gpu_ctx):
    """A shard of ONE window at n >= 2^24 (the 8-GPU case) runs as two half-size sub-MSMs over the point halves,
    added on the host: all K one-window shards must still combine to the full MSM."""
    n = 1 << 24
    gpu_ctx.generate_points(n, seed=77)
    dev, _ = gpu_ctx.generate_scalars(n, seed=78)
    full, info = gpu_ctx.run_device(dev, n, c=16)
    K = info["K"]
    parts = b"".join(gpu_ctx.window_sums(dev, n, k, k + 1, c=16, on_device=True)[0] for k in range(K))
    assert gpu_ctx.combine(parts, K, 16).as_tuple() == full.as_tuple()
    # two-window shards (4-GPU case) take the ordinary path
    parts2 = b"".join(gpu_ctx.window_sums(dev, n, k, k + 2, c=16, on_device=True)[0] for k in range(0, K, 2))
    assert parts2 == parts or gpu_ctx.combine(parts2, K, 16).as_tuple() == full.as_tuple()


def test_folded_top_window(gpu_ctx):
    """Windows of 18 and 21 bits on BLS12-377 (127 = 7 * 18 + 1 = 6 * 21 + 1; `msmProjective`: 254 = 11 * 23 + 1): the top window
    would hold the carry bit of the signed recoding alone, so the plan folds it into the window below -- one window less, the
    top one c + 1 bits wide and not recoded, weights 2^(c k) unchanged.  Same group element as the oracle and as the plain plan,
    through full MSMs, one-window shards + msm_combine, and scalars whose halves sit at the edges of the recoding."""
    from montgomery_amd.distributed import combine_host

    pts, _ = O.random_points_bls377("gpu/fold", 300)
    sc = O.prng_ints("gpu/fold/s", 300, C.q)
    gpu_ctx.set_points(O.points_to_bytes(pts, 48))
    exp = O.msm_batched_affine(sc, pts, c=16)
    for c, K in ((18, 7), (21, 6)):
        res, info = gpu_ctx.run(O.scalars_to_bytes(sc), c=c)
        assert (info["c"], info["K"]) == (c, K) and res.as_tuple() == exp, info
    for lg in (12, 18, 21):
        n = 1 << lg
        gpu_ctx.generate_points(n, seed=700 + lg)
        dev, _ = gpu_ctx.generate_scalars(n, seed=800 + lg)
        want, _ = gpu_ctx.run_device(dev, n, c=16)
        for c in (18, 21):
            got, info = gpu_ctx.run_device(dev, n, c=c)
            assert got.as_tuple() == want.as_tuple(), (lg, c, info)
            K = info["K"]
            parts = b"".join(gpu_ctx.window_sums(dev, n, k, k + 1, c=c, on_device=True)[0] for k in range(K))
            assert combine_host(parts, K, c) == want.as_tuple(), (lg, c)
    # every scalar the same: all entries of a window in one bucket; q - 1 and 2^252 - 1 drive the top window to its largest values
    n = 1 << 12
    gpu_ctx.generate_points(n, seed=99)
    for val in (C.q - 1, C.q - 2, 1, (1 << 252) - 1):
        sb = O.scalars_to_bytes([val] * n)
        want, _ = gpu_ctx.run(sb, c=16)
        for c in (18, 21):
            assert gpu_ctx.run(sb, c=c)[0].as_tuple() == want.as_tuple(), (hex(val), c)
    dev, _ = gpu_ctx.generate_scalars(n, seed=6)
    want, _ = gpu_ctx.run_device(dev, n)
    got, info = gpu_ctx.run_device(dev, n, c=23, no_glv=True)
    assert info["K"] == 11 and got.as_tuple() == want.as_tuple()
