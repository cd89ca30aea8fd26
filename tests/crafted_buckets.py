"""Buckets with chosen contents, for the last stages of every MSM: plain helpers, numpy and Python integers only, no fixtures,
no GPU.

Every MSM ends with the bucket finish (k_finish_hist / k_finish_perm, k_bucket_finish or k_te_bucket_finish: msm_tree.hip) and
the bucket reduction P_k = sum_l l B_(k,l) (reduce_buckets, msm_reduce.hip: k_bucket_reduce, the two k_bit_tree launches, the
host's double-and-add pass).  Whole MSMs over random scalars reach few of their branches and none of their hard inputs.  Here a
window group is written down bucket by bucket: Crafted holds a POOL of points k_j G with known k_j -- random points, their
negatives, the identity, small multiples of G -- and, as off / elems, the pool indices every bucket holds.  The expected window
sums follow from the discrete logs alone, one scaling of G per window whatever L is: Crafted.expected, Crafted.expected_group.
The named fill patterns at the end build the inputs of tests/test_gpu_bucket_sums.py (msm_test_bucket_sums, include/msm_hip.h);
tests/test_crafted_buckets.py proves them against the oracle's point arithmetic on the CPU first.
"""
import functools
import os
import sys

import numpy as np

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from degenerate_inputs import CURVE_TABLE  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

N_RANDOM = 14                         # pool: 14 random points, their 14 negatives, the identity, G, 2 G, -2 G
POOL = 2 * N_RANDOM + 4
IDENT, GEN = 2 * N_RANDOM, 2 * N_RANDOM + 1
DEEP_COUNTS = (0, 1, 2, 3, 7, 31, 32, 62, 63, 64)     # 64: the most the tree leaves in a bucket; 63 and 64 share the last bin
FINISH_BINS = 64                                      # tree_kernels.h


@functools.lru_cache(maxsize=None)
def base_pool(curve):
    """(points, logs) of the 32 pool points of a curve: j < 14 random, 14 + j = -(point j), then the identity, G, 2 G, -2 G."""
    cv = CURVE_TABLE[curve]
    if cv.te:
        pts, logs = O.random_points_ed377(f"buckets/{curve}", N_RANDOM)
    else:
        pts, logs = O.random_points_bls377(f"buckets/{curve}", N_RANDOM, cv.B)
    pts, logs = list(pts), list(logs)
    pts += [cv.neg(P) for P in pts]
    logs += [(cv.q - d) % cv.q for d in logs]
    pts += [cv.zero, cv.scale_g(1), cv.scale_g(2), cv.scale_g(cv.q - 2)]
    logs += [0, 1, 2, cv.q - 2]
    assert len(pts) == len(logs) == POOL and pts[GEN] == (cv.B.gx, cv.B.gy)
    return tuple(pts), tuple(logs)


def neg_index(j):
    """pool index of -(pool point j), for the random points and their negatives"""
    assert 0 <= j < 2 * N_RANDOM
    return j + N_RANDOM if j < N_RANDOM else j - N_RANDOM


class Crafted:
    """K windows of L buckets over a pool: bucket l (1-based) of window k holds the pool points elems[off[k L + l - 1] : off[k L + l]]."""

    def __init__(self, name, curve, K, L, counts, elems, extra=()):
        cv = CURVE_TABLE[curve]
        pts, logs = base_pool(curve)
        self.name, self.curve, self.cv, self.K, self.L = name, curve, cv, K, L
        self.points = list(pts) + [cv.scale_g(d) for d in extra]      # points of a chosen log, added behind the base pool
        self.logs = list(logs) + [d % cv.q for d in extra]
        counts = np.asarray(counts, dtype=np.int64)
        assert L & (L - 1) == 0 and counts.shape == (K * L,) and counts.min(initial=0) >= 0
        self.off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        self.elems = np.asarray(elems, dtype=np.uint32)
        assert self.elems.shape == (int(self.off[-1]),) and (len(self.elems) == 0 or int(self.elems.max()) < len(self.points))

    @property
    def counts(self):
        return np.diff(self.off.astype(np.int64))

    def pool_wire(self):
        """the pool as wire points: x || y; the identity as zeros on a Weierstrass curve, as (0, 1) on the Edwards curve"""
        return self.cv.wire(self.points)

    def bucket(self, k, l):
        """pool indices of bucket l (1 .. L) of window k"""
        b = k * self.L + l - 1
        return self.elems[self.off[b]:self.off[b + 1]].tolist()

    def window_logs(self):
        """[k] -> (sum_l l sum_(e in bucket (k, l)) d_e) mod q, from the discrete logs alone"""
        K, L, q = self.K, self.L, self.cv.q
        weight = np.repeat(np.tile(np.arange(1, L + 1, dtype=np.int64), K), self.counts)      # l of every element
        window = np.repeat(np.repeat(np.arange(K, dtype=np.int64), L), self.counts)
        per_point = np.zeros((K, len(self.points)), dtype=np.int64)                            # sum of l per (window, pool point): < 2^63
        np.add.at(per_point, (window, self.elems.astype(np.int64)), weight)
        return [sum(int(w) * d for w, d in zip(per_point[k].tolist(), self.logs)) % q for k in range(K)]

    def expected(self):
        """[k] -> P_k as an affine result (the identity: None, or (0, 1) on the Edwards curve)"""
        return [self.cv.scale_g(d) for d in self.window_logs()]

    def group_log(self, stride):
        return sum(d << (stride * k) for k, d in enumerate(self.window_logs())) % self.cv.q

    def expected_group(self, stride):
        """sum_k 2^(stride k) P_k: what a merged call owes"""
        return self.cv.scale_g(self.group_log(stride))


def decode_slots(cv, raw, K):
    """K x 144 bytes (X || Y || Z) -> affine results: Z = 0 is the identity of a Weierstrass curve; the Edwards identity is (0, 1)"""
    out = []
    for k in range(K):
        X, Y, Z = (int.from_bytes(raw[144 * k + 48 * j:144 * k + 48 * j + 48], "little") for j in range(3))
        assert max(X, Y, Z) < cv.p
        if Z == 0:
            assert not cv.te, "an extended Edwards point has Z != 0"
            out.append(None)
        else:
            zi = pow(Z, -1, cv.p)
            out.append((X * zi % cv.p, Y * zi % cv.p))
    return out


def horner(cv, slots, stride):
    """sum_k 2^(stride k) slots[k] with the curve's affine arithmetic"""
    acc = cv.zero
    for P in reversed(slots):
        acc = cv.add(cv.scale(1 << stride, acc) if acc != cv.zero else acc, P)
    return acc


# ---------------------------------------------------------------------------------------------- the fill patterns
# Every pattern is f(curve, K, L, tc=2, seed=...) -> Crafted; tc = buckets per chunk of the reduction (TC in reduce_buckets),
# for the patterns that speak of chunks: chunk ch of a window holds the buckets ch tc + 1 .. (ch + 1) tc.

def _rng(name, curve, K, L, seed):
    return np.random.default_rng([seed, K, L, sum(map(ord, name + curve))])


def random(curve, K, L, tc=2, seed=1):
    """0 to 3 elements per bucket, any pool point: negatives and identities among them"""
    rng = _rng("random", curve, K, L, seed)
    counts = rng.integers(0, 4, size=K * L)
    return Crafted("random", curve, K, L, counts, rng.integers(0, POOL, size=int(counts.sum())))


def one_point(curve, K, L, tc=2, seed=2):
    """every bucket holds the same single point: all row sums, chunk triangles and fold operands of a window are equal"""
    return Crafted("one_point", curve, K, L, np.ones(K * L, dtype=np.int64), np.full(K * L, 5))


def all_empty(curve, K, L, tc=2, seed=3):
    return Crafted("all_empty", curve, K, L, np.zeros(K * L, dtype=np.int64), [])


def one_window_empty(curve, K, L, tc=2, seed=4):
    """window 1 is empty, every bucket of the others holds 1 to 3 elements"""
    assert K >= 2
    rng = _rng("one_window_empty", curve, K, L, seed)
    counts = rng.integers(1, 4, size=K * L)
    counts[L:2 * L] = 0
    return Crafted("one_window_empty", curve, K, L, counts, rng.integers(0, POOL, size=int(counts.sum())))


def _single_buckets(name, curve, K, L, ls):
    """per window the buckets ls, one random pool point each (another per window and bucket), everything else empty"""
    counts = np.zeros(K * L, dtype=np.int64)
    elems = []
    for k in range(K):
        for i, l in enumerate(ls):
            counts[k * L + l - 1] = 1
            elems.append((3 * k + 5 * i) % (2 * N_RANDOM))
    return Crafted(name, curve, K, L, counts, elems)


def only_first(curve, K, L, tc=2, seed=5):
    return _single_buckets("only_first", curve, K, L, [1])


def only_last(curve, K, L, tc=2, seed=6):
    return _single_buckets("only_last", curve, K, L, [L])


def one_chunk(curve, K, L, tc=2, seed=7):
    """only the tc buckets of one chunk past the middle of every window are filled"""
    ch = (L // tc) * 2 // 3
    return _single_buckets("one_chunk", curve, K, L, list(range(ch * tc + 1, (ch + 1) * tc + 1)))


def cancel_in_chunk(curve, K, L, tc=2, seed=8):
    """P in the first bucket of every chunk and -P in the second: every row sum is the identity, reached halfway through the
    lane's chain; the chunk triangles are not"""
    assert tc >= 2 and L % tc == 0
    counts = np.zeros((K, L // tc, tc), dtype=np.int64)
    counts[:, :, :2] = 1
    j = (np.arange(L // tc) + np.arange(K)[:, None]) % (2 * N_RANDOM)
    elems = np.stack([j, np.where(j < N_RANDOM, j + N_RANDOM, j - N_RANDOM)], axis=2)
    return Crafted("cancel_in_chunk", curve, K, L, counts.ravel(), elems.ravel())


def cancel_chunk_pairs(curve, K, L, tc=2, seed=9):
    """the first bucket of chunk 2 i holds P_i, that of chunk 2 i + 1 holds -P_i: neighbouring row sums cancel, so every run of
    an even number of consecutive chunks (the A runs of the two-dimensional bit tree) sums to the identity"""
    nch = L // tc
    assert nch % 2 == 0
    counts = np.zeros((K, nch, tc), dtype=np.int64)
    counts[:, :, 0] = 1
    j = (np.arange(nch) // 2 + np.arange(K)[:, None]) % N_RANDOM
    elems = np.where(np.arange(nch) % 2 == 0, j, j + N_RANDOM)
    return Crafted("cancel_chunk_pairs", curve, K, L, counts.ravel(), elems.ravel())


def zero_window(curve, K, L, tc=2, seed=10):
    """window 0 sums to the identity: a random fill, and in bucket 1 one more point, of log -(sum of the rest) mod q"""
    rng = _rng("zero_window", curve, K, L, seed)
    counts = rng.integers(0, 4, size=K * L)
    counts[0] = 2
    elems = rng.integers(0, POOL, size=int(counts.sum()))
    rest = Crafted("zero_window", curve, K, L, counts, elems)
    q = rest.cv.q
    d = (-(rest.window_logs()[0] - rest.logs[int(elems[0])])) % q      # element 0 (bucket 1 of window 0, weight 1) is replaced
    elems[0] = POOL
    return Crafted("zero_window", curve, K, L, counts, elems, extra=(d,))


def deep(curve, K, L, tc=2, seed=11):
    """Deep buckets for the finish: the counts DEEP_COUNTS in turn, and inside them in turn one point repeated, P, -P, R
    repeated, and random points with the identity first, in the middle and last."""
    rng = _rng("deep", curve, K, L, seed)
    nb = K * L
    b = np.arange(nb)
    counts = np.asarray(DEEP_COUNTS, dtype=np.int64)[(b + b // len(DEEP_COUNTS)) % len(DEEP_COUNTS)]    # (the phase moves: every count meets every kind)
    kind = (b // len(DEEP_COUNTS)) % 3
    bucket = np.repeat(b, counts)
    pos = np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)          # position inside the bucket
    n = np.repeat(counts, counts)
    P = bucket % N_RANDOM
    R = (bucket * 5 + 3) % N_RANDOM
    rnd = rng.integers(0, 2 * N_RANDOM, size=len(bucket))
    same = P
    triple = np.choose(pos % 3, [P, P + N_RANDOM, R])
    idents = np.where((pos == 0) | (pos == n // 2) | (pos == n - 1), IDENT, rnd)
    elems = np.choose(np.repeat(kind, counts), [same, triple, idents])
    return Crafted("deep", curve, K, L, counts, elems)


PATTERNS = {f.__name__: f for f in (random, one_point, all_empty, one_window_empty, only_first, only_last, one_chunk, cancel_in_chunk,
                                    cancel_chunk_pairs, zero_window, deep)}


@functools.lru_cache(maxsize=64)
def make(pattern, curve, K, L, tc=2):
    return PATTERNS[pattern](curve, K, L, tc)
