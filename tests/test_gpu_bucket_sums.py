"""The last stages of every MSM on crafted buckets, through msm_test_bucket_sums (`-m gpu`): the bucket finish exactly as the
accumulation tree runs it (k_finish_hist / k_finish_perm from 4096 buckets, k_bucket_finish / k_te_bucket_finish, on bucket
sums that start out as garbage) and reduce_buckets on its output -- k_bucket_reduce / k_te_bucket_reduce, the two-dimensional
bit tree or the window sum, the host's double-and-add pass with `merged`, `stride` and every number of buckets per lane.

The inputs come from tests/crafted_buckets.py (proved on the CPU by tests/test_crafted_buckets.py); every expected value is one
scaling of G by a sum of known discrete logs, and every comparison is exact affine equality.

    shape                         reaches (buckets per lane TC = 2 by the library's rule while K L <= 2^17: nchunks = L / 2)
    K = 3,  L = 64                not bit-sliced (nchunks = 32 < 64): the lanes' weighting chains; finish without an order
    K = 65, L = 64                4160 >= 4096 buckets: the order of the finish, with a partial last block of 1024
    K = 1,  L = 128               nchunks = 64, nbits = 6: the smallest bit-sliced case, M_hi = M_lo = 8, nblk = 2
    K = 3,  L = 256               nbits = 7, odd: M_hi = 8, M_lo = 16
    K = 2,  L = 2^12              nbits = 11, nblk = 4, ordered finish; with TC = 4 .. 32: nchunks 1024 .. 128, `lt` of the host pass
    K = 1,  L = 2^14              nbits = 13: M_lo = 128 > 64 lanes
    K = 1,  L = 2^15              nbits = 14: M = 128 / 128, nblk = 32
    K = 4,  L = 2^16              2^18 buckets: the rule itself picks TC = 4
    K = 3,  L = 2^10 (Edwards)    three windows are not bit-sliced there: k_te_window_sum over 512 chunks, two per lane
"""
import numpy as np
import pytest

import crafted_buckets as B

pytestmark = pytest.mark.gpu

FINISH_ORDER_FROM = 4096      # buckets from which the finish orders them (msm_tree.hip)


def rule_tc(nb):
    """buckets per lane as reduce_buckets picks them for nb buckets (msm_reduce.hip)"""
    tc, cap = 2, (32 if nb >= 1 << 22 else 16)
    while tc < cap and nb // tc > 65536:
        tc *= 2
    return tc


def bit_sliced(cv, K, L, tc):
    TC = min(tc or rule_tc(K * L), L)
    return L // TC >= 64 and (not cv.te or K <= 2)


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


def run(ctx_of, cr, merged=False, stride=0, tc=0):
    """the decoded slots of one call; from 4096 buckets on also checks the order the finish took the buckets in"""
    K, L = cr.K, cr.L
    raw, perm = ctx_of(cr.curve).test_bucket_sums(cr.pool_wire(), cr.off, cr.elems, K, L, merged=merged, stride=stride, tc=tc, want_perm=True)
    perm = perm.astype(np.int64)
    if K * L >= FINISH_ORDER_FROM:
        # a permutation of the buckets, in descending order of their element counts (counts from 63 up share the last bin)
        assert (np.sort(perm) == np.arange(K * L)).all()
        keys = np.minimum(cr.counts[perm], B.FINISH_BINS - 1)
        assert (np.diff(keys) <= 0).all(), "the finish does not take the buckets in descending order of their counts"
    else:
        assert (perm == np.arange(K * L)).all()
    return B.decode_slots(cr.cv, raw, K)


def check_plain(ctx_of, cr, tc=0):
    got = run(ctx_of, cr, tc=tc)
    exp = cr.expected()
    assert got == exp, [k for k in range(cr.K) if got[k] != exp[k]]


def check_merged(ctx_of, cr, stride, tc=0):
    """sum_k 2^(stride k) slot_k is the group's sum; a bit-sliced call leaves it in slot 0 and the identity in the others"""
    cv = cr.cv
    got = run(ctx_of, cr, merged=True, stride=stride, tc=tc)
    assert B.horner(cv, got, stride) == cr.expected_group(stride)
    if bit_sliced(cv, cr.K, cr.L, tc):
        assert got[1:] == [cv.zero] * (cr.K - 1)


def ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def test_the_rule_for_buckets_per_lane_is_restated_rightly():
    assert [rule_tc(nb) for nb in (3 * 64, 1 << 17, (1 << 17) + 1, (1 << 17) + 2, 1 << 18, 1 << 21, 1 << 22)] == [2, 2, 2, 4, 4, 16, 32]
    cv = B.CURVE_TABLE["bls377"]
    assert not bit_sliced(cv, 3, 64, 0) and bit_sliced(cv, 1, 128, 0) and bit_sliced(cv, 2, 4096, 32) and not bit_sliced(cv, 2, 4096 // 4, 32)
    te = B.CURVE_TABLE["ed377"]
    assert bit_sliced(te, 2, 4096, 0) and not bit_sliced(te, 3, 1024, 0)


# ---------------------------------------------------------------------------------------------- every shape, random fill

# (curve, K, L, tc)
SHAPES = [("bls377", K, L, 0) for K, L in ((3, 64), (65, 64), (1, 128), (3, 256), (2, 1 << 12), (1, 1 << 14), (1, 1 << 15), (4, 1 << 16))]
SHAPES += [("bls377", 2, 1 << 12, tc) for tc in (4, 8, 16, 32)]
SHAPES += [("pallas", K, L, 0) for K, L in ((3, 64), (65, 64), (1, 128), (3, 256), (2, 1 << 12))] + [("pallas", 2, 1 << 12, 32)]
SHAPES += [("ed377", 1, 128, 0), ("ed377", 2, 1 << 12, 0), ("ed377", 2, 1 << 12, 32), ("ed377", 3, 1 << 10, 0)]


@pytest.mark.parametrize("curve,K,L,tc", SHAPES, ids=ids(SHAPES))
def test_random_buckets(ctx_of, curve, K, L, tc):
    check_plain(ctx_of, B.make("random", curve, K, L), tc)


# ---------------------------------------------------------------------------------------------- merged calls

# (curve, K, L, tc, stride): stride = log2 L + 1 is the plain plan, log2 L the plan with a folded top window (Weierstrass, K >= 2)
def _merged(curve, K, L, tc, fold=True):
    lg = L.bit_length() - 1
    return [(curve, K, L, tc, lg + 1)] + ([(curve, K, L, tc, lg)] if K >= 2 and fold else [])


MERGED = [c for K, L, tc in ((1, 128, 0), (3, 256, 0), (2, 1 << 12, 0), (2, 1 << 12, 32), (3, 64, 0)) for c in _merged("bls377", K, L, tc)]
MERGED += _merged("pallas", 3, 256, 0) + _merged("pallas", 2, 1 << 12, 32)
MERGED += _merged("ed377", 1, 128, 0) + _merged("ed377", 2, 1 << 12, 0, fold=False) + _merged("ed377", 2, 1 << 12, 32, fold=False)


@pytest.mark.parametrize("curve,K,L,tc,stride", MERGED, ids=ids(MERGED))
def test_merged_group_sum(ctx_of, curve, K, L, tc, stride):
    check_merged(ctx_of, B.make("random", curve, K, L), stride, tc)


@pytest.mark.parametrize("pattern", ["one_point", "cancel_chunk_pairs", "zero_window", "all_empty"])
@pytest.mark.parametrize("stride", [8, 9])
def test_merged_group_sum_of_degenerate_windows(ctx_of, pattern, stride):
    """the overlap of a folded top window (stride 8 = log2 L) with sums that are equal, cancel or are the identity"""
    check_merged(ctx_of, B.make(pattern, "bls377", 3, 256), stride)


# ---------------------------------------------------------------------------------------------- every fill pattern

PATTERN_CASES = [(curve, p, K, L) for curve, shapes in (("bls377", ((3, 256), (2, 1 << 12))), ("pallas", ((3, 256),)),
                                                        ("ed377", ((2, 1 << 12), (3, 1 << 10))))
                 for K, L in shapes for p in sorted(B.PATTERNS) if p != "random"]


@pytest.mark.parametrize("curve,pattern,K,L", PATTERN_CASES, ids=ids(PATTERN_CASES))
def test_fill_patterns(ctx_of, curve, pattern, K, L):
    assert rule_tc(K * L) == 2                   # the chunks the patterns speak of are the library's
    check_plain(ctx_of, B.make(pattern, curve, K, L, 2))


@pytest.mark.parametrize("pattern", ["one_chunk", "cancel_in_chunk", "cancel_chunk_pairs"])
def test_chunk_patterns_at_32_buckets_per_lane(ctx_of, pattern):
    check_plain(ctx_of, B.make(pattern, "bls377", 2, 1 << 12, 32), tc=32)


# ---------------------------------------------------------------------------------------------- the boundary

def test_arguments_are_checked(ctx_of):
    from montgomery_amd import MsmError

    ctx = ctx_of("bls377")
    cr = B.make("random", "bls377", 3, 64)

    def refused(**kw):
        a = dict(off=cr.off, elems=cr.elems, K=3, L=64, tc=0)
        a.update(kw)
        with pytest.raises(MsmError) as e:
            ctx.test_bucket_sums(cr.pool_wire(), a["off"], a["elems"], a["K"], a["L"], tc=a["tc"])
        assert e.value.code == 1

    for tc in (1, 3, 64):
        refused(tc=tc)
    off = cr.off.copy()
    off[5], off[6] = off[6] + 1, off[5]
    refused(off=off)
    elems = cr.elems.copy()
    elems[7] = len(cr.points)
    refused(elems=elems)
    refused(off=np.zeros(3 * 48 + 1, dtype=np.uint32), elems=[], L=48)
    check_plain(ctx_of, cr)                      # the context is as good as before
