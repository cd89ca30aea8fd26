"""The stage between "sorted" and "finished" on crafted bucket sizes, through msm_test_tree_sums (`-m gpu`): the scans behind the
sort (k_bucket_max, k_pscan_partial / _top / _final), the host's round plan in accumulate_window_group (FINISH_MAX,
tail_min_pairs, r_stop, the two alternating buffers, round_geom per round), k_tail_desc, and the rounds in their real order on
the real buffers -- the slot-form gather round 1 over padded slots, the regular rounds, the search rounds -- then the bucket
finish and the reduction.

Every case asserts, in this order: (1) the plan the library reports equals tests/tree_model.py (RT, r_stop, total_slots,
max_bucket, rounds, n_pairs, and the outputs of every launched round); (2) the device's cursor and all its tail_off tables equal
the model word for word; (3) the K window sums equal Crafted.expected() -- one scaling of G per window, from discrete logs -- by
affine equality.  The inputs come from tests/crafted_buckets.py (proved on the CPU by tests/test_crafted_buckets.py and
tests/test_tree_model.py).

G = 2^logG; F = FINISH_MAX = 32 for the class of c = 16 and 64 for that of c = 21.

    A  one bucket of F G, F G + 1, 2 F G, 2 F G + 1 entries among buckets of 0 to 3: r_stop 0, 1, 1, 2; logG 1, 2, 3, 5, 10, so
       that logG + r_stop is even and odd: both parities of the buffer alternation into the finish
    B  the buckets hold 0, 1, ..., 4 F G + G entries, in this order and in reverse
    C  the blocks of k_tail_desc: a bucket over three whole blocks and more, a bucket boundary on a block boundary behind a run
       of empty buckets, empty runs at both ends, 256 k and 256 k + 1 outputs, one bucket in all, the last bucket the deep one
    D  the scan blocks: 4096, 6144 and 3 * 4096 buckets with deep ones at the ends of every block and in the four buckets of one
       lane; 3 * 2^21 buckets (1536 scan blocks: the second trip of k_pscan_top)
    E  rounds of every mode with three or more pairs per lane and a ragged last block, read from the library's round log
    F  r_stop by the pair count: 2^17 buckets of 64 entries at logG = 1 leave 32 elements each, and the first tail round has 2^21
       outputs; one bucket of 60 makes it 2^21 - 1.  (The 2^23 of the class of c >= 18 needs 2^25 entries: left to the end-to-end tests.)
    G  A and C with the largest bucket over-reported 2 x and 64 x: RT grows, extra rounds mostly copy, the sums stay
    H  degenerate content deep enough for the tail rounds: doublings in every round, P - P in round 1 and in round 2, identity rows
    I  A and B with random payload bits (sign; beta x line on the Weierstrass curves)
    J  no entry, one entry, two entries in one bucket
"""
import time

import numpy as np
import pytest

import crafted_buckets as B
import tree_model as T

pytestmark = pytest.mark.gpu

CLASSES = {16: 32, 21: 64}                       # c -> F
OTHER_CURVES = ("pallas", "ed377")               # an 8-word Weierstrass curve and the Edwards curve: cases A, B, C, H, I
ALL_CURVES = ("bls377",) + OTHER_CURVES
TIMES = {}


@pytest.fixture(scope="module")
def ctx_of():
    from montgomery_amd.api import MsmContext

    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = MsmContext(B.CURVE_TABLE[curve].cid)
        return made[curve]

    yield get
    for c in made.values():
        c.close()
    slowest = sorted(TIMES.items(), key=lambda kv: -kv[1])[:5]
    print("\nslowest msm_test_tree_sums cases (s, model and expected values included):", [(k, round(v, 2)) for k, v in slowest])


def first_difference(got, want):
    bad = np.nonzero(np.asarray(got, dtype=np.int64) != want)
    return None if len(bad[0]) == 0 else tuple(int(a[0]) for a in bad)


def check(ctx_of, cr, logG, c, reported_max=0, label=""):
    t0 = time.perf_counter()
    plan = T.TreePlan(cr.counts, logG, c, reported_max)
    got = ctx_of(cr.curve).test_tree_sums(cr.pool_wire(), cr.off, cr.elems, cr.K, cr.L, c, logG, flags=cr.flags,
                                          reported_max=reported_max, tail_tables=plan.RT + 1)
    keys = ("RT", "r_stop", "total_slots", "max_bucket", "rounds", "n_pairs")
    print({k: got[k] for k in keys}, got["log"])
    # 1. the plan
    assert {k: got[k] for k in keys} == {k: getattr(plan, k) for k in keys}
    assert [(mode, n_out) for mode, n_out, _ in got["log"]] == plan.round_outputs
    # 2. the scans, word for word: (bucket) of the first wrong cursor, (round, bucket) of the first wrong offset
    bad = first_difference(got["cursor"], plan.cursor)
    assert bad is None, f"cursor: first wrong word at (bucket) {bad}"
    assert got["tail_off"].shape == plan.tail_off.shape
    bad = first_difference(got["tail_off"], plan.tail_off)
    assert bad is None, f"tail_off: first wrong word at (round, bucket) {bad}"
    # 3. the sums
    sums, exp = B.decode_slots(cr.cv, got["sums"], cr.K), cr.expected()
    assert sums == exp, [k for k in range(cr.K) if sums[k] != exp[k]]
    TIMES[f"{cr.name}-{cr.curve}-{label}-G{logG}-c{c}-m{reported_max}"] = time.perf_counter() - t0
    return got, plan


# ---------------------------------------------------------------------------------------------- A, G, I: the r_stop threshold

A_CASES = [(c, logG, i) for c in CLASSES for logG in (1, 2, 3, 5, 10) for i in range(4)]


def a_deep(c, logG, i):
    F, G = CLASSES[c], 1 << logG
    return ((F * G, 0), (F * G + 1, 1), (2 * F * G, 1), (2 * F * G + 1, 2))[i]


@pytest.mark.parametrize("flags", [False, True], ids=["plain", "flags"])
@pytest.mark.parametrize("c,logG,i", A_CASES)
@pytest.mark.parametrize("curve", ALL_CURVES)
def test_a_r_stop_threshold(ctx_of, curve, c, logG, i, flags):
    deep, r_stop = a_deep(c, logG, i)
    got, plan = check(ctx_of, B.tree_threshold(curve, deep, flags=flags), logG, c, label=f"A{i}")
    assert got["r_stop"] == r_stop and got["rounds"] == logG + r_stop


def test_a_both_parities_of_the_buffer_alternation_are_reached():
    assert {(logG + a_deep(c, logG, i)[1]) % 2 for c, logG, i in A_CASES} == {0, 1}


@pytest.mark.parametrize("over", [2, 64])
@pytest.mark.parametrize("c,logG,i", A_CASES)
def test_g_over_reported_maximum_at_the_threshold(ctx_of, c, logG, i, over):
    deep, r_stop = a_deep(c, logG, i)
    got, plan = check(ctx_of, B.tree_threshold("bls377", deep), logG, c, reported_max=over * deep, label=f"G{i}")
    assert got["RT"] == T.tail_rounds(over * deep, logG) > T.tail_rounds(deep, logG) and got["r_stop"] > r_stop


# ---------------------------------------------------------------------------------------------- B, I: every size once

@pytest.mark.parametrize("flags", [False, True], ids=["plain", "flags"])
@pytest.mark.parametrize("reverse", [False, True], ids=["up", "down"])
@pytest.mark.parametrize("logG", [1, 3])
@pytest.mark.parametrize("c", list(CLASSES))
@pytest.mark.parametrize("curve", ALL_CURVES)
def test_b_every_size_once(ctx_of, curve, c, logG, reverse, flags):
    F, G = CLASSES[c], 1 << logG
    got, plan = check(ctx_of, B.tree_every_size(curve, 4 * F * G + G, reverse, flags), logG, c, label="B")
    assert got["r_stop"] == 3


# ---------------------------------------------------------------------------------------------- C, G: the descriptor blocks

def c_cases(curve):
    """(label, pattern, logG): all at c = 16"""
    return [("blocks", B.tree_desc_blocks(curve, 0), 1), ("blocks+1", B.tree_desc_blocks(curve, 1), 1),
            ("one_bucket", B.tree_one_bucket(curve, 5001), 1), ("one_bucket_G8", B.tree_one_bucket(curve, 5001), 3),
            ("last_deep", B.tree_last_deep(curve, 777), 1)]


@pytest.mark.parametrize("case", range(5))
@pytest.mark.parametrize("curve", ALL_CURVES)
def test_c_descriptor_blocks(ctx_of, curve, case):
    label, cr, logG = c_cases(curve)[case]
    got, plan = check(ctx_of, cr, logG, 16, label=label)
    assert got["r_stop"] >= 1
    if case < 2:      # the first search round has 256 k (+ 1) outputs
        assert [n for mode, n, _ in got["log"] if mode == "search"][0] % B.TREE_BLOCK == case


@pytest.mark.parametrize("over", [2, 64])
@pytest.mark.parametrize("case", range(5))
def test_g_over_reported_maximum_over_descriptor_blocks(ctx_of, case, over):
    label, cr, logG = c_cases("bls377")[case]
    true_max = int(cr.counts.max())
    got, plan = check(ctx_of, cr, logG, 16, reported_max=over * true_max, label=label)
    assert got["RT"] > T.tail_rounds(true_max, logG) and got["max_bucket"] == over * true_max


# ---------------------------------------------------------------------------------------------- D: the scan blocks

@pytest.mark.parametrize("K,L", [(1, 4096), (3, 2048), (3, 4096)])
def test_d_scan_blocks(ctx_of, K, L):
    got, plan = check(ctx_of, B.tree_scan_blocks("bls377", K, L), 1, 16, label="D")
    assert got["r_stop"] >= 1


def test_d_second_trip_of_the_top_scan(ctx_of):
    K, L = 3, 1 << 21
    assert -(-K * L // T.PS_SPAN) == 1536 > T.SCAN_THREADS
    cr = B.tree_sparse("bls377", K, L)
    assert 300 <= np.count_nonzero(cr.counts) <= 500
    got, plan = check(ctx_of, cr, 1, 16, label="D2")
    assert got["r_stop"] == 1


# ---------------------------------------------------------------------------------------------- E: steps

def test_e_rounds_of_three_and_more_pairs_per_lane(ctx_of):
    got, plan = check(ctx_of, B.tree_steps("bls377"), 2, 16, label="E")
    for mode in ("gather", "regular", "search"):
        assert any(m == mode and steps >= 3 and n_out % (256 * steps) for m, n_out, steps in got["log"]), (mode, got["log"])


# ---------------------------------------------------------------------------------------------- F: stopping by the pair count

@pytest.mark.parametrize("odd_one,r_stop", [(0, 1), (60, 0)])
def test_f_r_stop_by_the_pair_count(ctx_of, odd_one, r_stop):
    got, plan = check(ctx_of, B.tree_equal("bls377", 1 << 17, 64, odd_one), 1, 16, label="F")
    assert plan.tail_tot[1] == (1 << 21) - (1 if odd_one else 0) and int(plan.counts.max()) == 64 == 32 << 1
    assert got["r_stop"] == r_stop


# ---------------------------------------------------------------------------------------------- H: degenerate content

@pytest.mark.parametrize("logG", [1, 3])
@pytest.mark.parametrize("c", list(CLASSES))
@pytest.mark.parametrize("curve", ALL_CURVES)
def test_h_degenerate_content_at_every_level(ctx_of, curve, c, logG):
    cr = B.tree_degenerate(curve, 1024)
    assert 1024 > CLASSES[c] << logG
    got, plan = check(ctx_of, cr, logG, c, label="H")
    assert got["r_stop"] >= 1


# ---------------------------------------------------------------------------------------------- J: nothing and almost nothing

@pytest.mark.parametrize("curve", ALL_CURVES)
def test_j_nothing_and_almost_nothing(ctx_of, curve):
    cv = B.CURVE_TABLE[curve]
    got, plan = check(ctx_of, B.all_empty(curve, 2, 8), 1, 16, label="J")
    assert (got["total_slots"], got["rounds"], got["n_pairs"], got["log"]) == (0, 0, 0, [])
    assert B.decode_slots(cv, got["sums"], 2) == [cv.zero] * 2
    for entries in (1, 2):
        got, plan = check(ctx_of, B.tree_few(curve, entries), 1, 16, label=f"J{entries}")
        assert (got["total_slots"], got["rounds"], got["n_pairs"]) == (2, 1, 1)


# ---------------------------------------------------------------------------------------------- the boundary

def test_arguments_are_checked(ctx_of):
    from montgomery_amd import MsmError
    from montgomery_amd.api import MsmContext

    ctx = ctx_of("bls377")
    cr = B.tree_threshold("bls377", 65)

    def refused(on=ctx, **kw):
        a = dict(off=cr.off, elems=cr.elems, K=2, L=64, c=16, logG=1, flags=None, reported_max=0)
        a.update(kw)
        with pytest.raises(MsmError) as e:
            on.test_tree_sums(cr.pool_wire(), a["off"], a["elems"], a["K"], a["L"], a["c"], a["logG"], flags=a["flags"],
                              reported_max=a["reported_max"])
        assert e.value.code == 1
        check(ctx_of, cr, 1, 16, label="again")             # the context is as good as before

    multi = MsmContext(devices=[0, 0])
    try:
        refused(on=multi)
    finally:
        multi.close()
    off = cr.off.copy()
    off[5], off[6] = off[6] + 1, off[5]
    refused(off=off)
    off = cr.off.copy()
    off[0] = 1
    refused(off=off)
    elems = cr.elems.copy()
    elems[7] = len(cr.points)
    refused(elems=elems)
    for logG in (0, 11):
        refused(logG=logG)
    for c in (0, 25):
        refused(c=c)
    refused(reported_max=64)
    refused(off=np.zeros(2 * 48 + 1, dtype=np.uint32), elems=[], L=48)          # the sizes msm_test_bucket_sums refuses
    refused(flags=np.full(len(cr.elems), 4, dtype=np.uint8))
    te = B.tree_threshold("ed377", 65)
    with pytest.raises(MsmError) as e:                                          # no beta x line on the Edwards curve
        ctx_of("ed377").test_tree_sums(te.pool_wire(), te.off, te.elems, 2, 64, 16, 1, flags=np.full(len(te.elems), 2, dtype=np.uint8))
    assert e.value.code == 1
    check(ctx_of, te, 1, 16, label="again")
