"""Every global access of k_batch_add and of the bin split goes through the two helpers of mem_policy.h, which carry the cache
policy of their stream (batch_add.h BaPol, sort_kernels.h SortPol, msm_kernels.h DigPol).  A policy says where bytes are cached,
never what they are: each case here runs one instantiated access path at the smallest shape that reaches it and compares the
result with (sum s_i a_i mod q) G for points of known discrete logs, or with the crafted buckets' expected sums.

    gather round, slot form       2^18 points at c = 18 (pair list read, rows gathered, planes out; the prefix scratch of 13 limbs)
    gather round, pair form       2^21 points at c = 18 under a lowered msm_test_set_chunk_rows_log: `dest`, records out and records
                                  read back by round 2 -- two records per element (BLS12-377), one record [x | y] (BN254), and the
                                  prefix plane of 9 limbs = two 16-byte pieces + one dword (Pallas)
    regular and search rounds     three and more pairs per lane and a ragged last block, read from the library's round log
    in-place round                the all-affine bucket reduction, whose sums replace their first operand
    the sort's paths              one level, radix split, bin split into slots, bin split into pairs, by the library's own report

Needs an MI355X: `-m gpu`."""
import pytest

import crafted_buckets as B
import crafted_digits as D
from degenerate_inputs import CURVE_TABLE
from oracle import msm_oracle as O
from test_gpu_pair_form import rows_log, uniform

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx_of(gpu_ctx):
    from montgomery_amd.api import MsmContext

    made = {"bls377": gpu_ctx}

    def get(curve):
        if curve not in made:
            made[curve] = MsmContext(CURVE_TABLE[curve].cid)
        return made[curve]

    yield get
    for name, c in made.items():
        if name != "bls377":
            c.close()


def run_and_check(ctx, cv, c_oracle, n, seed, c, want_paths, **kw):
    a, dev, s, exp = uniform(ctx, cv, n, seed, c_oracle)
    res, info = ctx.run_device(dev, n, c=c, **kw)
    paths = ctx.test_last_sort_paths()
    print(cv.name, n, paths, {k: info[k] for k in ("c", "K", "tables", "rounds", "max_bucket")})
    assert paths == want_paths, paths
    assert res.as_tuple() == exp, info
    return info


def test_slot_form_gather(gpu_ctx, c_oracle):
    info = run_and_check(gpu_ctx, CURVE_TABLE["bls377"], c_oracle, 1 << 18, 3100, 18, ["slots"], no_tables=True)
    assert (info["c"], info["tables"]) == (18, False)


@pytest.mark.parametrize("name", ["bls377", "bn254", "pallas"])
def test_pair_form_records_out_and_in(ctx_of, c_oracle, name):
    ctx, n = ctx_of(name), D.PAIR_MIN_PLAIN[18]
    with rows_log(ctx, D.PAIR_ROWS_LOG):
        info = run_and_check(ctx, CURVE_TABLE[name], c_oracle, n, 3200, 18, ["pairs"], no_tables=True)
    assert info["rounds"] >= 2          # round 1 writes the records, round 2 reads them back (logG = 2 at this size)


@pytest.mark.parametrize("curve", ["bls377", "pallas"])
def test_regular_and_search_rounds_of_three_and_more_steps(ctx_of, curve):
    cr = B.tree_steps(curve)
    got = ctx_of(curve).test_tree_sums(cr.pool_wire(), cr.off, cr.elems, cr.K, cr.L, 16, 2, flags=cr.flags)
    print(got["log"])
    for mode in ("gather", "regular", "search"):
        assert any(m == mode and steps >= 3 and n_out % (256 * steps) for m, n_out, steps in got["log"]), (mode, got["log"])
    assert B.decode_slots(cr.cv, got["sums"], cr.K) == cr.expected()


def test_in_place_round_of_the_all_affine_reduction(gpu_ctx):
    C = O.BLS12_377
    K, L = 2, 64
    pts, _ = O.random_points_bls377("stream-policy/reduce", K * L)
    pts[7] = pts[70] = None
    pts[20] = pts[21]                                       # P + P inside the in-place rounds
    buckets = b"".join(bytes(96) if P is None else P[0].to_bytes(48, "little") + P[1].to_bytes(48, "little") for P in pts)
    exp = []
    for k in range(K):
        acc = None
        for l in range(1, L + 1):
            if pts[k * L + l - 1] is not None:
                acc = O.aff_add(acc, O.aff_scale(l, pts[k * L + l - 1], C.p), C.p)
        exp.append(acc)

    def affine(parts):
        out = []
        for k in range(K):
            X, Y, Z = (int.from_bytes(parts[144 * k + 48 * j: 144 * k + 48 * j + 48], "little") for j in range(3))
            out.append(None if Z == 0 else (X * pow(Z, -1, C.p) % C.p, Y * pow(Z, -1, C.p) % C.p))
        return out

    for c0 in (0, 2):                                       # the tree alone; chunks of four buckets
        got, _ = gpu_ctx.test_bucket_reduce(buckets, K, L, mode=1, c0=c0)
        assert affine(got) == exp, c0


@pytest.mark.parametrize("n,c,path", [(4096, None, "one_level"), (D.RADIX_N, 16, "radix")])
def test_sort_paths_below_the_bin_split(gpu_ctx, c_oracle, n, c, path):
    """(the bin split's two forms are the slot-form and pair-form cases above)"""
    info = run_and_check(gpu_ctx, CURVE_TABLE["bls377"], c_oracle, n, 3300, c, [path], no_tables=True)
    assert c is None or info["c"] == c
