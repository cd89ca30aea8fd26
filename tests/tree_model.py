"""The stage between "sorted" and "finished" of a window group, restated in Python integers and numpy: plain helpers, no
fixtures, no GPU.

What the library computes there, and where:
    the scans behind the sort     k_bucket_max, k_pscan_partial / _top / _final (sort_kernels.h): per bucket of n entries and the
                                  padding granule G = 2^logG the quantities q = 0: roundup(n, G) (-> cursor, the slot a bucket
                                  starts at) and q = 1 + r: ceil(ceil(n / G) / 2^r) for r = 0 .. RT (-> tail_off[r], the element a
                                  bucket starts at after r tail rounds), each with its total
    the host's round plan         accumulate_window_group (msm_tree.hip): FINISH_MAX and tail_min_pairs by the window class, the
                                  tail rounds r_stop that run, the rounds and pair additions msm_result reports
    the tail-round descriptors    k_tail_desc (tree_kernels.h): output e of tail round r -> (first operand, second present)
TreePlan holds all of it for one vector of bucket sizes; tests/test_tree_model.py proves it by running the whole tree on
integers, tests/test_gpu_tree.py compares msm_test_tree_sums with it word for word.
"""
import numpy as np

PS_ITEMS, PS_BLOCK = 4, 1024          # buckets per lane and lanes per block of the scans
PS_SPAN = PS_ITEMS * PS_BLOCK         # buckets per scan block
SCAN_THREADS = 1024                   # scan blocks k_pscan_top takes per trip


def scan_quantity(n, logG, q):
    """quantity q of a bucket of n entries (numpy array or int): q = 0 its padded slots, q = 1 + r its elements after r tail rounds"""
    cg = (n + ((1 << logG) - 1)) >> logG
    if q == 0:
        return cg << logG
    r = q - 1
    return (cg + ((1 << r) - 1)) >> r


def tail_rounds(max_bucket, logG):
    """RT: the tail rounds that leave one element of the largest bucket, 2^RT >= ceil(max_bucket / G)"""
    capmax = (max_bucket + (1 << logG) - 1) >> logG
    rt = 0
    while rt < 32 and (1 << rt) < capmax:
        rt += 1
    return rt


def pscan_nq(max_bucket, logG):
    return tail_rounds(max_bucket, logG) + 2


def thresholds(c):
    """(FINISH_MAX, tail_min_pairs) of a plan of window c"""
    return (64, 1 << 23) if c >= 18 else (32, 1 << 21)


def _exclusive(v):
    return np.concatenate([[0], np.cumsum(v, dtype=np.int64)])


class TreePlan:
    """Everything between the bucket sizes `counts` (all windows of the group in a row) and the finish, for the padding granule
    2^logG and the threshold class of window c.  reported_max: what stands in for the largest bucket where the sort over-reports
    it (0: the true maximum)."""

    def __init__(self, counts, logG, c, reported_max=0):
        counts = np.asarray(counts, dtype=np.int64)
        self.counts, self.logG, self.c, self.nb = counts, logG, c, len(counts)
        true_max = int(counts.max(initial=0))
        assert reported_max == 0 or reported_max >= true_max
        self.max_bucket = reported_max or true_max
        self.RT = tail_rounds(self.max_bucket, logG)
        self.cursor = _exclusive(scan_quantity(counts, logG, 0))                                  # [nb + 1]
        self.total_slots = int(self.cursor[-1])
        self.tail_off = np.stack([_exclusive(scan_quantity(counts, logG, 1 + r)) for r in range(self.RT + 1)])   # [RT + 1][nb + 1]
        self.tail_tot = [int(t[-1]) for t in self.tail_off]                                        # info[3 + r]
        self.FINISH_MAX, self.tail_min_pairs = thresholds(c)
        cap_elems = (self.max_bucket + (1 << logG) - 1) >> logG                                   # of the largest bucket behind the regular rounds
        r_stop = 0
        while r_stop < self.RT and (((cap_elems + (1 << r_stop) - 1) >> r_stop) > self.FINISH_MAX
                                    or self.tail_tot[r_stop + 1] >= self.tail_min_pairs):
            r_stop += 1
        self.r_stop = r_stop
        # round r = 1 .. logG halves the slots; tail round r = 1 .. r_stop writes tail_tot[r] elements
        self.round_outputs = ([("gather" if r == 1 else "regular", self.total_slots >> r) for r in range(1, logG + 1)]
                              + [("search", self.tail_tot[r]) for r in range(1, r_stop + 1)]) if self.total_slots else []
        self.rounds = len(self.round_outputs)
        self.n_pairs = sum(n for _, n in self.round_outputs)

    def desc(self, r):
        """descriptors of tail round r = 1 .. RT: (index of the first operand among the elements of round r - 1, second operand
        present), one per output element"""
        off_in, off_out = self.tail_off[r - 1], self.tail_off[r]
        n_out = np.diff(off_out)
        bucket = np.repeat(np.arange(self.nb, dtype=np.int64), n_out)
        j = np.arange(int(off_out[-1]), dtype=np.int64) - off_out[bucket]
        ia = off_in[bucket] + 2 * j
        return ia, ia + 1 < off_in[bucket + 1]

    def desc_words(self, r):
        """the words k_tail_desc writes: (first operand << 1) | present"""
        ia, present = self.desc(r)
        return ((ia << 1) | present).astype(np.uint32)


def simulate(plan, values):
    """The whole tree on integers.  values: one integer per entry, the entries of bucket b in a row at [sum(counts[:b]), ...).
    Regular rounds add neighbouring slots, tail rounds add by the plan's descriptors, the finish adds what is left.
    Returns (bucket sums, elements every bucket holds when the finish takes over)."""
    counts, G = plan.counts, 1 << plan.logG
    values = np.asarray(values, dtype=np.int64)
    start = _exclusive(counts)
    assert len(values) == int(start[-1])
    x = np.zeros(plan.total_slots, dtype=np.int64)                     # pads are absent operands: they add nothing
    bucket = np.repeat(np.arange(plan.nb, dtype=np.int64), counts)
    x[plan.cursor[bucket] + np.arange(len(values)) - start[bucket]] = values
    for _ in range(plan.logG):
        x = x[0::2] + x[1::2]
    assert len(x) == plan.tail_tot[0] and (plan.cursor == plan.tail_off[0] * G).all()
    for r in range(1, plan.r_stop + 1):
        ia, present = plan.desc(r)
        assert len(ia) == plan.tail_tot[r] and (len(ia) == 0 or int(ia.max()) < len(x))
        second = np.where(present, x[np.minimum(ia + 1, len(x) - 1)], 0) if len(x) else np.zeros(0, dtype=np.int64)
        x = x[ia] + second
    off = plan.tail_off[plan.r_stop]
    assert len(x) == int(off[-1])
    csum = _exclusive(x)
    return csum[off[1:]] - csum[off[:-1]], np.diff(off)
