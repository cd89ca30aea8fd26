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
A Crafted may also carry one flag byte per element (negate, beta x line), and the tree_* patterns at the very end choose bucket
SIZES for the accumulation tree: the inputs of tests/test_gpu_tree.py (msm_test_tree_sums).
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

    def __init__(self, name, curve, K, L, counts, elems, extra=(), flags=None):
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
        # per element, for the entries that take them (msm_test_tree_sums): bit 0 negates the point, bit 1 takes the beta x line of
        # its row -- the element then stands for -d, lambda d or -lambda d
        self.flags = None if flags is None else np.asarray(flags, dtype=np.uint8)
        assert self.flags is None or (self.flags.shape == self.elems.shape and int(self.flags.max(initial=0)) <= (1 if cv.te else 3))

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
        kind = np.zeros(len(self.elems), dtype=np.int64) if self.flags is None else self.flags.astype(np.int64)
        per_point = np.zeros((K, 4, len(self.points)), dtype=np.int64)                         # sum of l per (window, flags, pool point): < 2^63
        np.add.at(per_point, (window, kind, self.elems.astype(np.int64)), weight)
        factor = (1, -1) if self.cv.te else (1, -1, self.cv.B.lam, -self.cv.B.lam)             # what the flags make of a log
        return [sum(f * sum(int(w) * d for w, d in zip(per_point[k, i].tolist(), self.logs) if w) for i, f in enumerate(factor)) % q
                for k in range(K)]

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


# ---------------------------------------------------------------------------------------------- the fill patterns of the tree
# For msm_test_tree_sums (tests/test_gpu_tree.py): what matters here is how many entries every bucket holds.  F = FINISH_MAX of
# the window class (32 below c = 18, 64 from it), G = 2^logG the padding granule: a bucket of n entries holds ceil(n / G)
# elements behind the regular rounds, and tail rounds run while the largest holds more than F.  flags: also give every element
# random payload bits (negate; on the Weierstrass curves the beta x line too).

def _tree(name, curve, K, L, counts, elems=None, flags=False, seed=0):
    """a Crafted over the counts; elems = None: any pool point per entry"""
    counts = np.asarray(counts, dtype=np.int64)
    rng = _rng(name, curve, K, L, seed)
    n = int(counts.sum())
    if elems is None:
        elems = rng.integers(0, POOL, size=n)
    fl = rng.integers(0, 2 if CURVE_TABLE[curve].te else 4, size=n).astype(np.uint8) if flags else None
    return Crafted(name, curve, K, L, counts, elems, flags=fl)


def tree_threshold(curve, deep, flags=False, bucket=64 + 37):
    """K = 2, L = 64: one bucket of `deep` entries among buckets of 0 to 3 (A: deep = F G, F G + 1, 2 F G, 2 F G + 1)"""
    counts = _rng("tree_threshold", curve, 2, 64, deep).integers(0, 4, size=128)
    counts[bucket] = deep
    return _tree("tree_threshold", curve, 2, 64, counts, flags=flags, seed=deep)


def tree_every_size(curve, top, reverse=False, flags=False):
    """K = 1: the buckets hold 0, 1, 2, ..., top entries in this order (or in reverse), the rest of the window is empty
    (B: top = 4 F G + G, so every tail level meets every small size, the odd ones with their missing second operand)"""
    L = 1 << (top + 1).bit_length()
    counts = np.zeros(L, dtype=np.int64)
    counts[:top + 1] = np.arange(top + 1)[::-1] if reverse else np.arange(top + 1)
    return _tree("tree_every_size", curve, 1, L, counts, flags=flags, seed=top + int(reverse))


TREE_BLOCK = 256       # outputs per block of k_tail_desc
TREE_EMPTY_RUN = 300   # empty buckets in a row: more than a block has lanes


def tree_desc_blocks(curve, extra=0):
    """C, at logG = 1 (a bucket of n entries holds ceil(n / 2) elements behind the regular round and ceil(n / 4) outputs in the
    first tail round), K = 1, L = 2048:
        300 empty buckets | A: 1024 entries = 256 outputs, so the next bucket starts a block | 300 empty buckets, which that block
        boundary falls into | D: 4400 entries = 1100 outputs, three whole blocks and more inside one bucket | 100 buckets of 1 to 3 |
        single entries until the first tail round has 256 k + `extra` outputs | empty to the end (more than 300)"""
    L, run = 2048, TREE_EMPTY_RUN
    rng = _rng("tree_desc_blocks", curve, 1, L, extra)
    counts = np.zeros(L, dtype=np.int64)
    counts[run] = 4 * TREE_BLOCK
    d = 2 * run + 1
    counts[d] = 4400
    counts[d + 1:d + 101] = rng.integers(1, 4, size=100)
    outputs = int(((counts + 3) // 4).sum())
    fill = (extra - outputs) % TREE_BLOCK
    counts[d + 101:d + 101 + fill] = 1
    assert d + 101 + fill + run <= L
    return _tree("tree_desc_blocks", curve, 1, L, counts, seed=extra)


def tree_one_bucket(curve, deep):
    """K = 1, L = 1: the whole group is one deep bucket"""
    return _tree("tree_one_bucket", curve, 1, 1, [deep], seed=deep)


def tree_last_deep(curve, deep):
    """K = 1, L = 64: buckets of 0 to 3, the last one alone is deep"""
    counts = _rng("tree_last_deep", curve, 1, 64, deep).integers(0, 4, size=64)
    counts[-1] = deep
    return _tree("tree_last_deep", curve, 1, 64, counts, seed=deep)


TREE_SCAN_SPAN, TREE_SCAN_ITEMS = 4096, 4     # buckets per block and per lane of the scans (PS_SPAN, PS_ITEMS)


def tree_scan_blocks(curve, K, L, deep=65):
    """D: buckets of 0 to 3; deep buckets (deep, deep + 1, ... entries) at the first and last bucket of every block of 4096 buckets
    and at each of the four buckets of one lane (lane 77 of block 0)"""
    nb = K * L
    counts = _rng("tree_scan_blocks", curve, K, L, deep).integers(0, 4, size=nb)
    at = sorted({b for b0 in range(0, nb, TREE_SCAN_SPAN) for b in (b0, min(b0 + TREE_SCAN_SPAN, nb) - 1)}
                | {77 * TREE_SCAN_ITEMS + j for j in range(TREE_SCAN_ITEMS)})
    counts[at] = deep + np.arange(len(at))
    return _tree("tree_scan_blocks", curve, K, L, counts, seed=deep)


def tree_sparse(curve, K, L, every=4 * TREE_SCAN_SPAN, deep=70):
    """D, the second trip of k_pscan_top: one bucket of 1 to 3 entries every `every` buckets and in the last bucket, all else empty;
    two deep buckets, one in the first scan block and one behind the 1024 scan blocks of the first trip"""
    nb = K * L
    counts = np.zeros(nb, dtype=np.int64)
    at = np.concatenate([np.arange(every // 2, nb, every), [nb - 1]])
    counts[at] = _rng("tree_sparse", curve, K, L, deep).integers(1, 4, size=len(at))
    counts[5] = deep
    counts[min(nb - 2, 1024 * TREE_SCAN_SPAN + TREE_SCAN_SPAN + 3)] = deep + 1
    return _tree("tree_sparse", curve, K, L, counts, seed=deep)


def tree_steps(curve, L=1 << 18, filled=150_000, per=4, deep=1001):
    """E: `filled` buckets of `per` entries and one deep bucket of an odd size: rounds of a few hundred thousand outputs"""
    counts = np.zeros(L, dtype=np.int64)
    counts[:filled] = per
    counts[filled + 7] = deep
    return _tree("tree_steps", curve, 1, L, counts, seed=deep)


def tree_equal(curve, nb, per, odd_one=0):
    """F: nb buckets of `per` entries each; odd_one: the size of bucket 1000 instead"""
    counts = np.full(nb, per, dtype=np.int64)
    if odd_one:
        counts[1000] = odd_one
    return _tree("tree_equal", curve, 1, nb, counts, elems=np.resize(np.arange(2 * N_RANDOM), int(counts.sum())), seed=odd_one)


def tree_degenerate(curve, n=1024):
    """H, K = 1, L = 8, n a power of two: bucket 1 holds n copies of one point (a doubling in every round), 2: P, -P, P, -P, ...
    (round 1 cancels, identities from then on), 3: P, P, -P, -P, ... (round 2 cancels), 4: a point and the pool's identity row in
    turn, 5: identity rows alone, 6: three entries, 7 and 8: empty"""
    P = 3
    i = np.arange(n)
    buckets = [np.full(n, P), np.where(i % 2 == 0, P, neg_index(P)), np.where(i % 4 < 2, P, neg_index(P)),
               np.where(i % 2 == 0, i // 2 % N_RANDOM, IDENT), np.full(n, IDENT), np.array([1, 2, IDENT]), i[:0], i[:0]]
    return _tree("tree_degenerate", curve, 1, 8, [len(b) for b in buckets], elems=np.concatenate(buckets))


def tree_few(curve, entries):
    """J, K = 2, L = 8: nothing, one entry in all, or two entries in one bucket"""
    counts = np.zeros(16, dtype=np.int64)
    counts[11] = entries
    return _tree("tree_few", curve, 2, 8, counts, elems=[4, 9][:entries])
