"""Scalars with chosen window digits, for the sort's heavy-bin parts and path switches: plain helpers, numpy and Python
integers only, no fixtures, no GPU.

Every MSM entry point sorts its window digits in sort_window_group (montgomery_amd/csrc/msm_sort.hip), on one of three paths
(one level, radix split, bin split) whose choice and whose inner cuts -- coarse bins, the parts of heavy bins -- depend on how
the digits are distributed.  Random, repeated and prover-like scalars reach few of those cuts.  Here a scalar is put together
from the signed digits its windows shall have: scalar_from_digits; for the curves with an endomorphism the two halves are
crafted and glv_scalar folds them into one scalar whose decomposition gives them back (below a bound per curve: HALF_BITS).

An input is a POOL of distinct crafted scalars, exact counts per pool entry and an explicit point order: Crafted.  The named
distributions at the end build the shapes of the table in their docstrings; expected_stats gives the bucket histogram, the
largest bucket and the pair additions the library must report, from the crafted digits alone.
tests/test_crafted_digits.py proves all of it against the oracle before tests/test_gpu_sort_shapes.py relies on it.
"""
import os
import sys

import numpy as np

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from degenerate_inputs import CURVE_TABLE  # noqa: E402

# Largest bit length of a crafted non-negative GLV half for which (k1 + lambda k2) mod q decomposes back into (k1, k2) with
# both signs positive.  Found on the CPU with O.glv_decompose over 2 000 random pairs of halves of exactly that many bits:
#   BLS12-377: 120, 123, 124, 125 bits 2000 / 2000; 126 bits 9 (0.75 % in another draw); 127 bits 0
#   BN254 G1 : 118 .. 125 bits 2000 / 2000; 126 bits 1107; 127 bits 0
# (the lattice basis has 127-bit vectors: halves up to a quarter of them stay inside the rounding's fundamental cell)
HALF_BITS = {"bls377": 125, "bn254": 125}
TE_SCALAR_BITS = 250   # Ed-on-BLS12-377 has no endomorphism: a scalar below 2^250 < q reaches the digits as it is


def scalar_from_digits(digits, c):
    """sum e_k 2^(c k) for signed digits |e_k| <= 2^(c-1); a magnitude of exactly 2^(c-1) only as a positive digit
    (O.signed_digits recodes l > L as negative, so l = L stays positive)."""
    L = 1 << (c - 1)
    s = 0
    for k, e in enumerate(digits):
        e = int(e)
        assert -L < e <= L, (k, e)
        s += e << (c * k)
    return s


def glv_scalar(k1, k2, curve):
    """(k1 + lambda k2) mod q for crafted non-negative halves below 2^HALF_BITS[curve]."""
    B = CURVE_TABLE[curve].B
    assert 0 <= k1 < (1 << HALF_BITS[curve]) and 0 <= k2 < (1 << HALF_BITS[curve])
    return (k1 + B.lam * k2) % B.q


class Plan:
    """The window plan of one call, from the arithmetic of make_plan (include/msm_hip.h, montgomery_amd/csrc/msm_plan.hip):
    K = ceil((b + 1) / c), one window less where the carry bit alone would fill the top one (fold: c >= 18, not Edwards).
    narrow_bits: a narrow call (msm_run_narrow) of that many magnitude bits -- no endomorphism, b = narrow_bits."""

    def __init__(self, curve, c, narrow_bits=0):
        cv = CURVE_TABLE[curve]
        self.curve, self.cv, self.c, self.te, self.narrow = curve, cv, c, cv.te, bool(narrow_bits)
        b = narrow_bits or cv.scalar_bits
        self.bits = b + 1
        self.K = -(-self.bits // c)
        self.fold = (not cv.te) and c >= 18 and self.K > 1 and self.bits - (self.K - 1) * c == 1
        if self.fold:
            self.K -= 1
        if not narrow_bits:
            assert self.K == cv.plan_k(c)
        self.L_log = c if self.fold else c - 1
        self.halves = 1 if (cv.te or narrow_bits) else 2            # crafted digit strings per scalar
        self.per_point = 1 if cv.te else 2                          # entries per point and window (two_n_d / n)
        # (a curve without a measured HALF_BITS has the plan arithmetic and the sort's cuts only: no crafted scalars)
        self.value_bits = narrow_bits or (TE_SCALAR_BITS if cv.te else HALF_BITS.get(curve))
        if self.value_bits is not None:
            assert self.value_bits > c * (self.K - 1) + 2, "the crafted values do not reach the top window"
            self.top_max = 1 << (self.value_bits - c * (self.K - 1))    # top digits 1 .. top_max (top_max: with a negative digit below)
            assert self.top_max <= (1 << (c - 1))

    def eff_bits(self, k, tables=False):
        """Bits the bucket indices of window k really have (msm_sort.hip, the loop that fills WinSplit)."""
        if tables:
            return self.L_log
        top = k % self.K == self.K - 1
        return max(1, min(self.L_log, self.bits - k * self.c) if top else min(self.L_log, self.c - 1))

    def window_groups(self, n, tables=False):
        """[k_lo, k_hi) of the window groups of a call over n points with room for all of them (window_sums_once,
        window_groups_wanted in msm_internal.h): two groups from 2^22 points, on window tables from 2^21 (Edwards 2^20)."""
        two = self.K >= 2 and (n >= (1 << 22) or (tables and n >= (1 << 20 if self.te else 1 << 21)))
        wpg = -(-self.K // (2 if two else 1))
        return [(k, min(self.K, k + wpg)) for k in range(0, self.K, wpg)]


class Geometry:
    """The cuts of sort_geometry for windows [k_lo, k_hi) over n points, restated once from msm_plan.hip: the sort path
    (`fits_lds` .. `radix`, `will_chunk`), the split of every window's bucket index into coarse and fine bits
    (`abk = eff <= ab_big ? eff : max(ab_big, eff - BS_MAX_FB)`, `ws.fb = eff - abk`; the radix split: 7 fine bits), the bins of
    the group V = kc * hb, and `part_len = max(2^16, roundup(2 * n_entries / V, BP_TILE))` with BP_TILE = 4096.
    tables: the kc_d digit windows are one merged window of kc_d * two_n_d entries.
    chunk_rows: the table rows above which round 1 takes the pair form -- 2^23 unless a test has moved the context's threshold
    (msm_test_set_chunk_rows_log).  mean, logG: the mean bucket the padding granule is sized from, and log2 of that granule.
    tests/test_sort_geometry.py checks this restatement against the library's own sort_geometry (msm_plan.hip), on the CPU, over
    both curve kinds, every window and size: the GPU tests that build their inputs from it do not find out first."""

    def __init__(self, plan, n, k_lo, k_hi, tables=False, chunk_rows=1 << 23):
        kc_d = k_hi - k_lo
        two_n_d = plan.per_point * n
        self.n_entries = kc_d * two_n_d
        kc = 1 if tables else kc_d
        two_n = self.n_entries if tables else two_n_d
        L = 1 << plan.L_log
        fits_lds = L * 4 <= 128 * 1024
        limit = (1 << 22) if plan.te else (1 << 21)                 # one_level_entry_limit
        bin_split = (not fits_lds) or (tables and two_n >= (1 << 22))
        radix = (not bin_split) and plan.L_log > 7 and two_n >= limit and plan.L_log - 7 <= 8
        self.ab, self.fb = [], []
        for kk in range(kc):
            eff = plan.eff_bits(k_lo + kk, tables)
            if bin_split:
                ab = eff if eff <= 10 else max(10, eff - 12)
            else:
                ab = max(plan.L_log - 7, 0)             # (a window of fewer than 7 bits has no coarse ones)
                eff = plan.L_log
            self.ab.append(ab)
            self.fb.append(eff - ab)
        self.hb = max(1 << a for a in self.ab)
        self.V = kc * self.hb
        self.part_len = max(1 << 16, -(-(2 * self.n_entries // self.V) // 4096) * 4096) if bin_split else 0
        mean = max(1, two_n // (L // 2 if plan.fold else L))
        left = 32 if mean >= 512 else 16 if (mean >= 128 or (mean >= 64 and plan.c >= 18 and not tables)) else 8
        logG = 1
        while logG < 10 and (1 << (logG + 1)) * left <= mean:
            logG += 1
        self.mean, self.logG = mean, logG
        self.rows = rows = kc_d * n if tables else n
        pairs = bin_split and (not plan.te) and plan.c >= 18 and rows > chunk_rows and logG >= 2
        self.path = "pairs" if pairs else "slots" if bin_split else "radix" if radix else "one_level"


def fine_bits(plan, n, k, tables=False):
    """(fb, part_len) of digit window k of a call over n points: the group that holds it."""
    for lo, hi in plan.window_groups(n, tables):
        if lo <= k < hi:
            g = Geometry(plan, n, lo, hi, tables)
            return g.fb[0 if tables else k - lo], g.part_len
    raise AssertionError(k)


def expected_stats(pool_digits, counts, c, K, merged=None, keep=None):
    """From the crafted digits alone: (bucket histograms, largest bucket, sum of max(size - 1, 0)) -- the last is what
    info["n_pairs_algo"] reports.  pool_digits: (pool, halves, K) signed digits; counts: points per pool entry.
    hist[w][l] = entries of magnitude l in window w (l = 0: no entry, left out of the other two figures).
    merged: [(k_lo, k_hi)] -- a run on window tables, where the windows of a group share one set of buckets: one histogram per
    group.  keep: per window (lo, hi), only the bucket indices l - 1 in [lo, hi) (a bucket-range shard)."""
    pool_digits = np.asarray(pool_digits)
    assert pool_digits.shape[2] == K
    counts = np.asarray(counts, dtype=np.int64)
    size = int(np.abs(pool_digits).max()) + 1
    assert size <= (1 << c) + 1
    per_window = []
    for k in range(K):
        mag = np.abs(pool_digits[:, :, k]).astype(np.int64)
        w = np.broadcast_to(counts[:, None], mag.shape)
        h = np.bincount(mag.ravel(), weights=w.ravel().astype(np.float64), minlength=size).astype(np.int32)
        if keep is not None:
            lo, hi = keep[k]
            h[1:1 + lo] = 0
            h[1 + hi:] = 0
        per_window.append(h)
    hists = per_window if merged is None else [sum(per_window[lo + 1:hi], per_window[lo].copy()) for lo, hi in merged]
    largest = max(int(h[1:].max()) for h in hists)
    pairs = sum(int(np.maximum(h[1:].astype(np.int64) - 1, 0).sum()) for h in hists)
    return hists, largest, pairs


def shard_ranges(plan, g, G):
    """Bucket-index range [lo, hi) per window of shard g of G (make_plan, msm_opts.bucket_shards): the g-th of G equal parts of
    the span the digits cover, the last part to the end of the window's buckets."""
    L = 1 << plan.L_log
    top_bits = plan.c if plan.fold else min(plan.c - 1, plan.bits - (plan.K - 1) * plan.c)

    def cut(span):
        return span * g // G, (L if g + 1 == G else span * (g + 1) // G)

    low = cut(1 << (plan.c - 1) if plan.K > 1 else 1 << max(0, top_bits))
    return [low] * (plan.K - 1) + [cut(1 << max(0, top_bits))]


# ---------------------------------------------------------------------------------------------- one crafted input

class Crafted:
    """plan, n; digits (pool, halves, K) signed; counts (pool,) with sum n; order (n,): pool index of every point.
    bins {(window, bin): records} and buckets {(window, bin): populated buckets} are the structural claims of the distribution,
    which tests/test_crafted_digits.py checks against the histogram; on window tables `window` is the first window of the group
    whose merged window holds the bin.  fb, part_len {window: ...}: the cuts the sort applies to that digit window."""

    def __init__(self, name, plan, n, digits, counts, order, bins, buckets, fb, part_len, tables):
        self.name, self.plan, self.n, self.digits, self.counts, self.order = name, plan, n, digits, counts, order
        self.bins, self.buckets, self.fb, self.part_len, self.tables = bins, buckets, fb, part_len, tables
        self._pool = None

    def halves(self):
        """[pool][half] -> the crafted half scalars as Python integers."""
        c = self.plan.c
        return [[scalar_from_digits(d, c) for d in entry] for entry in self.digits.tolist()]

    def pool_scalars(self):
        if self._pool is None:
            hs = self.halves()
            self._pool = [glv_scalar(h[0], h[1], self.plan.curve) for h in hs] if self.plan.halves == 2 else [h[0] for h in hs]
        return self._pool

    def pool_bytes(self):
        return np.frombuffer(b"".join(s.to_bytes(32, "little") for s in self.pool_scalars()), dtype=np.uint8).reshape(-1, 32)

    def scalars(self, width=32):
        """The call's n x width byte array (width < 32: the low bytes, for a narrow call)."""
        return np.ascontiguousarray(self.pool_bytes()[self.order][:, :width])

    def merged(self):
        """The window groups of a run on window tables (expected_stats' `merged`), None on the plain path."""
        return self.plan.window_groups(self.n, True) if self.tables else None

    def stats(self, keep=None):
        return expected_stats(self.digits, self.counts, self.plan.c, self.plan.K, self.merged(), keep)

    def windows_of(self, window):
        """The digit windows whose entries share the buckets of `window`: itself, or its group on window tables."""
        if not self.tables:
            return [window]
        return [k for lo, hi in self.plan.window_groups(self.n, True) if lo <= window < hi for k in range(lo, hi)]

    def bin_records(self, window, b):
        """Bucket magnitudes of the records of bin b of (the merged window of) `window`, in record order: by digit window, by
        point, then by half."""
        fb = self.fb[window]
        out = []
        for k in self.windows_of(window):
            d = np.abs(self.digits[:, :, k])[self.order].ravel()
            out.append(d[(d > 0) & (((d - 1) >> fb) == b)])
        return np.concatenate(out)


def split_counts(total, m):
    """m counts as equal as possible that add up to total."""
    out = np.full(m, total // m, dtype=np.int64)
    out[:total % m] += 1
    return out


class Plant:
    """Half `half` of the entries [lo, hi) of a class gets, in digit window `window`, a digit of bin `b`: bucket offsets `offs`
    inside the bin (one per entry), negative where `neg` -- and where the digit allows it (not the top window's, not 2^(c-1))."""

    def __init__(self, window, b, offs, neg=None, half=0, lo=0, hi=None):
        self.window, self.b, self.offs, self.neg, self.half, self.lo, self.hi = window, b, np.asarray(offs, dtype=np.int64), neg, half, lo, hi


class Class:
    """m pool entries with counts (its points anywhere in the point order) or seq (its points in this order, as indices
    0 .. m - 1 into the class).  lone: no other entry shares a bucket with any digit of these entries."""

    def __init__(self, m, plants, counts=None, seq=None, lone=False):
        self.m, self.plants, self.lone = m, plants, lone
        self.seq = None if seq is None else np.asarray(seq, dtype=np.int64)
        self.counts = np.bincount(self.seq, minlength=m).astype(np.int64) if counts is None else np.asarray(counts, dtype=np.int64)
        assert len(self.counts) == m


def craft(name, plan, n, classes, seed, pool=4096, tables=False):
    """classes + uniform fill -> Crafted.  Fill digits are uniform over a window's signed digits (top window: 1 .. top_max - 1)
    and never fall into a bin that a plant names; fill entries share the points the classes leave.  The point order is a seeded
    permutation, in which the points of a class with `seq` keep the order seq gives them."""
    rng = np.random.default_rng(seed)
    c, K, H = plan.c, plan.K, plan.halves
    L = 1 << (c - 1)
    cuts = {k: fine_bits(plan, n, k, tables) for k in range(K)}
    fb = {k: cuts[k][0] for k in range(K)}
    part_len = {k: cuts[k][1] for k in range(K)}
    groups = plan.window_groups(n, True) if tables else [(k, k + 1) for k in range(K)]
    first_of = {k: lo for lo, hi in groups for k in range(lo, hi)}
    used = sum(int(cl.counts.sum()) for cl in classes)
    n_class = sum(cl.m for cl in classes)
    assert used <= n, (name, used, n)
    n_fill = min(max(pool - n_class, 64), n - used)
    P = n_class + n_fill
    digits = np.empty((P, H, K), dtype=np.int64)
    planted = np.zeros((P, H, K), dtype=bool)

    def draw(k, size):
        if k == K - 1:
            return rng.integers(1, plan.top_max, size=size)
        return rng.integers(-(L - 1), L + 1, size=size)

    for k in range(K):
        digits[:, :, k] = draw(k, (P, H))
    bins, reserved = {}, {}
    counts = np.zeros(P, dtype=np.int64)
    lone_rows = np.zeros(P, dtype=bool)
    at = 0
    for cl in classes:
        counts[at:at + cl.m] = cl.counts
        lone_rows[at:at + cl.m] = cl.lone
        for pt in cl.plants:
            lo, hi = pt.lo, cl.m if pt.hi is None else pt.hi
            k = pt.window
            assert len(pt.offs) == hi - lo and pt.offs.min() >= 0 and pt.offs.max() < (1 << fb[k]), (name, k)
            mag = (pt.b << fb[k]) + pt.offs + 1
            top = k == K - 1
            assert mag.max() <= (plan.top_max if top else L), (name, k, int(mag.max()))
            neg = np.zeros(hi - lo, dtype=bool) if pt.neg is None else np.asarray(pt.neg, dtype=bool)
            neg = neg & (mag < L) & (not top)
            rows = slice(at + lo, at + hi)
            assert not planted[rows, pt.half, k].any()
            digits[rows, pt.half, k] = np.where(neg, -mag, mag)
            planted[rows, pt.half, k] = True
            if top and K > 1:
                # a top digit of exactly top_max keeps the value below 2^value_bits only over a negative digit
                full = np.nonzero(mag == plan.top_max)[0] + at + lo
                assert not planted[full, pt.half, K - 2].any()
                digits[full, pt.half, K - 2] = -np.maximum(1, np.abs(digits[full, pt.half, K - 2]) % L)
                planted[full, pt.half, K - 2] = True
            key = (first_of[k], pt.b)
            bins[key] = bins.get(key, 0) + int(cl.counts[lo:hi].sum())
            for kk in range(*[g for g in groups if g[0] == first_of[k]][0]):
                reserved.setdefault(kk, set()).add(pt.b)
        at += cl.m
    # fill digits stay out of the planted bins, and out of the buckets of the `lone` entries
    for k in range(K):
        barr = np.array(sorted(reserved.get(k, ())), dtype=np.int64)
        while True:
            d = digits[:, :, k]
            free = ~planted[:, :, k] & ~lone_rows[:, None]
            hit = free & (d != 0) & np.isin((np.abs(d) - 1) >> fb[k], barr)
            if lone_rows.any():
                # (on window tables the windows of a group share their buckets: the lone digits of all of them count)
                glo, ghi = [g for g in groups if g[0] == first_of[k]][0]
                hit |= free & np.isin(np.abs(d), np.abs(digits[lone_rows, :, glo:ghi]))
            if not hit.any():
                break
            d[hit] = draw(k, int(hit.sum()))
    if n_fill:
        counts[n_class:] = split_counts(n - used, n_fill)
    assert counts.sum() == n
    buckets = {}
    for (k0, b) in bins:
        mags = []
        for k in range(*[g for g in groups if g[0] == k0][0]):
            d = np.abs(digits[:, :, k])
            mags.append(d[(d > 0) & (((d - 1) >> fb[k]) == b) & (counts[:, None] > 0)])
        buckets[(k0, b)] = len(np.unique(np.concatenate(mags)))
    # the point order
    pos = rng.permutation(n)
    order = np.empty(n, dtype=np.int64)
    at = taken = 0
    for cl in classes:
        m_pts = int(cl.counts.sum())
        where = pos[taken:taken + m_pts]
        if cl.seq is not None:
            order[np.sort(where)] = cl.seq + at
        else:
            order[where] = np.repeat(np.arange(at, at + cl.m), cl.counts)
        taken += m_pts
        at += cl.m
    order[pos[taken:]] = np.repeat(np.arange(n_class, P), counts[n_class:])
    return Crafted(name, plan, n, digits, counts, order, bins, buckets, fb, part_len, tables)


# ---------------------------------------------------------------------------------------------- the named distributions

def _alt_neg(m):
    return (np.arange(m) // 2) % 2 == 1


def _target(plan, n, window, b, tables=False):
    """(window, bin, fine bits, part_len): a middle window and a middle bin that the window's digits reach, unless given."""
    K = plan.K
    window = (K // 2 if K > 2 else 0) if window is None else window
    fb, part_len = fine_bits(plan, n, window, tables)
    reach = (plan.top_max if window == K - 1 else 1 << (plan.c - 1)) >> fb     # bins the digits of the window reach
    b = max(1, reach // 2 - 3) if b is None else b
    assert b < reach
    return window, b, fb, part_len


def full_bin(plan, n, window=None, b=None, seed=1, pool=4096, tables=False):
    """One middle bin holds 3 * part_len + 1 records over ALL 2^fb of its buckets, with both digit signs in every bucket.
    (Where the sort has no parts -- c <= 16 -- part_len stands for 2^16 and the bin is a coarse bin of the radix split.)"""
    window, b, fb, part_len = _target(plan, n, window, b, tables)
    NB = 1 << fb
    m = max(2 * NB, 1024)
    i = np.arange(m)
    cl = Class(m, [Plant(window, b, i % NB, neg=(i // NB) % 2 == 1)], counts=split_counts(3 * (part_len or 1 << 16) + 1, m))
    return craft("full_bin", plan, n, [cl], seed, max(pool, m + 1024), tables)


def exact_edges(plan, n, window=None, seed=2, pool=4096, bins=None, tables=False):
    """Four bins of one window hold exactly 2 * part_len, part_len + 1, 2 * part_len - 1 and part_len records.  With an
    endomorphism the entries of the second and fourth are entries of the first and third, through their other half (one half
    per point would not fit four such bins into 2^18 points).  bins: the four bins, else four around the middle one."""
    window, b0, fb, part_len = _target(plan, n, window, None, tables)
    bs = bins or [b0, b0 + 1, b0 + 3, b0 + 4]
    NB = 1 << fb
    m = max(NB, 64)
    offs = np.arange(m) % NB
    sizes = [2 * part_len, part_len + 1, 2 * part_len - 1, part_len]
    if plan.halves == 2:
        def pair(big, small, b_big, b_small):
            ms = m // 2
            cnt = np.concatenate([split_counts(small, ms), split_counts(big - small, m - ms)])
            return Class(m, [Plant(window, b_big, offs, _alt_neg(m)), Plant(window, b_small, offs[:ms], ~_alt_neg(ms), half=1, hi=ms)], counts=cnt)
        classes = [pair(sizes[0], sizes[1], bs[0], bs[1]), pair(sizes[2], sizes[3], bs[2], bs[3])]
    else:
        classes = [Class(m, [Plant(window, bb, offs, _alt_neg(m))], counts=split_counts(sz, m)) for sz, bb in zip(sizes, bs)]
    cr = craft("exact_edges", plan, n, classes, seed, pool, tables)
    assert [cr.bins[(cr.windows_of(window)[0], bb)] for bb in bs] == sizes
    return cr


def ends(plan, n, seed=3, pool=4096):
    """Bin 0 of window 0 and the last bin the digits reach in the last window (of the last group) are each multi-part; the
    bucket of the largest top digit, top_max -- 2^(c-1) where the values fill the top window's recoded range -- is populated."""
    K = plan.K
    fb0, pl0 = fine_bits(plan, n, 0)
    fbt, plt = fine_bits(plan, n, K - 1)
    assert fbt > 0
    last = (plan.top_max - 1) >> fbt
    m0, mt = 1 << fb0, plan.top_max - (last << fbt)
    if plan.halves == 2:
        # one class: its first halves in bin 0 of window 0, its second halves in the last bin (two classes of one half each
        # would need more than 2^18 points)
        m = max(m0, mt)
        both = Class(m, [Plant(0, 0, np.arange(m) % m0, _alt_neg(m)), Plant(K - 1, last, np.arange(m) % mt, half=1)],
                     counts=split_counts(2 * max(pl0, plt) + 3, m))
        return craft("ends", plan, n, [both], seed, pool)
    first = Class(m0, [Plant(0, 0, np.arange(m0), _alt_neg(m0))], counts=split_counts(2 * pl0 + 3, m0))
    top = Class(mt, [Plant(K - 1, last, np.arange(mt))], counts=split_counts(2 * plt + 5, mt))
    return craft("ends", plan, n, [first, top], seed, pool)


def neighbours(plan, n, seed=4, pool=4096, tables=False):
    """Three multi-part bins in EVERY window of every window group, two of them adjacent.  One class of part_len + 1 points has
    its first halves in bin b and its second halves in bin b + 1 of all K windows, another of 2 * part_len + 3 points its first
    halves in bin b + 3 (three classes of one half each would need more than 2^18 points).  On window tables the three bins
    are the same in all windows, so the merged window of a group holds its windows' records of them together."""
    K = plan.K
    assert plan.halves == 2
    m = 256
    cuts = [fine_bits(plan, n, k, tables) for k in range(K)]
    longest = max(pl for _, pl in cuts)

    def plants(half, shift):
        out = []
        for k in range(K):
            fb = cuts[k][0]
            reach = ((plan.top_max - 1) if (k == K - 1 or tables) else 1 << (plan.c - 1)) >> fb
            assert reach >= 8, (k, reach)
            out.append(Plant(k, reach // 2 + shift, (np.arange(m) * 7 + k + half) % (1 << fb), _alt_neg(m), half=half))
        return out

    classes = [Class(m, plants(0, 0) + plants(1, 1), counts=split_counts(longest + 1, m)),
               Class(m, plants(0, 3), counts=split_counts(2 * longest + 3, m))]
    return craft("neighbours", plan, n, classes, seed, pool, tables)


def _four_buckets(plan, n, window, b, tables=False):
    window, b, fb, part_len = _target(plan, n, window, b, tables)
    NB = 1 << fb
    assert NB >= 8
    return window, b, part_len, np.array([0, NB // 3, NB // 2 + 1, NB - 1])


def alternating(plan, n, window=None, b=None, seed=5, pool=4096, tables=False):
    """A heavy bin over four buckets A B C D in three parts and a bit.  In point order a full part is (A B C D) x (part_len / 4 - 1)
    and then B D B D: part_len / 4 - 1 entries of A and of C, part_len / 4 + 1 of B and of D -- EVERY part holds an odd count of
    every bucket.  The short last part is A B D.  (On window tables the bin holds no record of the group's other windows: the
    fill stays out of it in all of them.)"""
    window, b, part_len, offs = _four_buckets(plan, n, window, b, tables)
    part = np.concatenate([np.tile(np.arange(4), part_len // 4 - 1), np.array([1, 3, 1, 3])])
    seq = np.concatenate([part, part, part, np.array([0, 1, 3])])
    cl = Class(4, [Plant(window, b, offs, neg=[False, True, False, True])], seq=seq)
    return craft("alternating", plan, n, [cl], seed, pool, tables)


def runs(plan, n, window=None, b=None, seed=6, pool=4096):
    """A heavy bin of 3 * part_len + 1 records over four buckets, the point order sorted by bucket: the parts hold disjoint
    buckets but for the one bucket that straddles each part boundary."""
    window, b, part_len, offs = _four_buckets(plan, n, window, b)
    sizes = [part_len - 1001, part_len + 500, part_len + 300, 202]
    assert sum(sizes) == 3 * part_len + 1
    cl = Class(4, [Plant(window, b, offs, neg=[True, False, True, False])], seq=np.repeat(np.arange(4), sizes))
    return craft("runs", plan, n, [cl], seed, pool)


def giant_and_singletons(plan, n, window=None, b=None, seed=7, pool=4096):
    """One heavy bin holds one giant bucket (2 * part_len + 1 entries), every other bucket of the bin exactly 1, 2 or 3."""
    window, b, fb, part_len = _target(plan, n, window, b)
    NB = 1 << fb
    cnt = 1 + np.arange(NB) % 3
    cnt[NB // 2] = 2 * part_len + 1
    cl = Class(NB, [Plant(window, b, np.arange(NB), _alt_neg(NB))], counts=cnt)
    return craft("giant_and_singletons", plan, n, [cl], seed, max(pool, NB + 1024))


def short_top(plan, n, seed=8, pool=4096):
    """A plan whose top window has at most 10 bits (pass A sorts it outright: fb = 0, bin = bucket): every entry of the top
    window is in one of two top digits -- a third of the first halves and half of the second halves in the lower one."""
    K = plan.K
    assert fine_bits(plan, n, K - 1)[0] == 0 and plan.top_max >= 8
    m = pool
    d0, d1 = plan.top_max // 2, plan.top_max - 3
    z = np.zeros(m, dtype=np.int64)
    plants = [Plant(K - 1, d0 - 1, z[:m // 3], hi=m // 3), Plant(K - 1, d1 - 1, z[m // 3:], lo=m // 3)]
    if plan.halves == 2:
        plants += [Plant(K - 1, d1 - 1, z[:m // 2], half=1, hi=m // 2), Plant(K - 1, d0 - 1, z[m // 2:], half=1, lo=m // 2)]
    return craft("short_top", plan, n, [Class(m, plants, counts=split_counts(n, m))], seed, m)


def radix_edge(plan, n, m_largest, window=None, seed=9, pool=4096):
    """The largest bucket holds exactly m_largest entries: one pool entry with that count, whose digits no other entry shares
    (each of its digits is a bucket of m_largest entries; all others are far smaller)."""
    window, b, fb, _ = _target(plan, n, window, None)
    return craft("radix_edge", plan, n, [Class(1, [Plant(window, b, [5])], counts=[m_largest], lone=True)], seed, pool)


def radix_fat_bin(plan, n, window=None, seed=10):
    """One coarse bin holds half of a window's entries -- one half of EVERY point -- over all 2^fb of its buckets, evenly: no
    bucket above n / 2^fb (2^13 at 2^20 points)."""
    window, b, fb, _ = _target(plan, n, window, None)
    assert plan.halves == 2
    NB = 1 << fb
    m = 8 * NB
    cl = Class(m, [Plant(window, b, np.arange(m) % NB, _alt_neg(m))], counts=split_counts(n, m))
    return craft("radix_fat_bin", plan, n, [cl], seed, m)


# ---------------------------------------------------------------------------------------------- the cases of the GPU tests

DISTS = {"full_bin": full_bin, "exact_edges": exact_edges, "ends": ends, "neighbours": neighbours, "alternating": alternating,
         "runs": runs, "giant_and_singletons": giant_and_singletons, "short_top": short_top, "radix_edge": radix_edge,
         "radix_fat_bin": radix_fat_bin}

SLOT_N = (1 << 18, (1 << 18) + 77)
PAIR_N = (1 << 23) + 4096           # more than 2^23 table rows: the tile-ordered round 1 (will_chunk in msm_sort.hip)
PAIR_C = 18                         # ... which also wants logG >= 2: at this n the mean bucket of c = 21 is 16, too shallow
TABLES_N = (1 << 21) + 4096         # four shared window tables (c = 18, K = 7, two groups): 4 n > 2^23 rows
RADIX_N = 1 << 20
NARROW_BITS = 125                   # 16-byte narrow scalars: six unfolded 21-bit windows


class Case:
    """One crafted input of tests/test_gpu_sort_shapes.py: make() builds it (once: the CPU and the GPU module share the cache)."""
    _made = {}

    def __init__(self, dist, curve="bls377", c=21, n=1 << 18, narrow_bits=0, tables=False, **kw):
        self.dist, self.curve, self.c, self.n, self.narrow_bits, self.tables, self.kw = dist, curve, c, n, narrow_bits, tables, kw
        extra = "".join(f"-{k}{'_'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in sorted(kw.items()) if k != "pool")
        self.id = f"{dist}-{curve}{'-narrow' if narrow_bits else ''}{'-tables' if tables else ''}-c{c}-n{n}{extra}".replace(" ", "")

    def make(self):
        if self.id not in Case._made:
            if len(Case._made) >= 4:      # (a 2^23-point case holds 64 MB of point order)
                Case._made.pop(next(iter(Case._made)))
            plan = Plan(self.curve, self.c, self.narrow_bits)
            kw = dict(self.kw)
            if self.tables:
                kw["tables"] = True
            Case._made[self.id] = DISTS[self.dist](plan, self.n, **kw)
        return Case._made[self.id]


_TRIO = ("full_bin", "exact_edges", "giant_and_singletons")
SLOT_CASES = [cs for n in SLOT_N for cs in
              [Case(d, c=21, n=n) for d in ("full_bin", "exact_edges", "ends", "neighbours", "alternating", "runs", "giant_and_singletons")]
              + [Case(d, c=c, n=n) for c in (18, 24) for d in _TRIO] + [Case("short_top", c=20, n=n)]]
PAIR_CASES = [Case(d, c=PAIR_C, n=PAIR_N, pool=16384) for d in ("full_bin", "exact_edges", "alternating", "runs", "giant_and_singletons", "ends")]
TABLES_CASES = [Case(d, c=18, n=TABLES_N, tables=True, pool=8192) for d in ("full_bin", "neighbours")]
RADIX_CASES = ([Case("radix_edge", c=16, n=RADIX_N, m_largest=m) for m in ((1 << 17) - 1, 1 << 17)] + [Case("radix_fat_bin", c=16, n=RADIX_N)]
               + [Case("full_bin", c=16, n=n) for n in (RADIX_N - 1, RADIX_N)])
ED_CASES = [Case(d, curve="ed377", c=21, n=1 << 19) for d in ("full_bin", "exact_edges")]
NARROW_CASE = Case("full_bin", c=21, n=1 << 18, narrow_bits=NARROW_BITS)
INDEXED_CASE = Case("full_bin", c=21, n=1 << 18, seed=11)
# bucket shards (g, 2) of a 21-bit plan cut every window's 2^20 buckets at 2^19 = the start of bin 512
SHARD_CASES = [Case("full_bin", c=21, n=1 << 18, b=300), Case("exact_edges", c=21, n=1 << 18, bins=(510, 511, 512, 513))]
BN254_CASE = Case("full_bin", curve="bn254", c=21, n=1 << 18)

# ---------------------------------------------------------------------------------------------- the pair form at small sizes
# tests/test_gpu_pair_form.py lowers the context's row threshold (msm_test_set_chunk_rows_log) to 2^PAIR_ROWS_LOG rows; what is
# left of `will_chunk` in msm_sort.hip is c >= 18 and logG >= 2.  logG >= 2 means 4 * per_bucket_left <= mean, and
# per_bucket_left is 8 below a mean of 64: mean >= 32.  The mean is floor(entries of the (merged) window / 2^(c-1)) -- a folded
# plan fills L / 2 = 2^(c-1) of its 2^c buckets, an unfolded one has L = 2^(c-1) -- and a window holds 2 n entries on the plain
# path (both GLV halves; no_glv and narrow calls keep the second, empty, half), 2 n kc_d on window tables that merge kc_d windows:
#     plain   n >= 2^(c+3)                    c = 18: 2^21, c = 21: 2^24, c = 22: 2^25
#     tables  n kc_d >= 2^(c+3); below 2^21 points one group of all K windows, from 2^21 two groups and the smaller one has
#             floor(K / 2) windows            c = 18: K = 7: ceil(2^21 / 7) = 299 594, K = 8: 2^18
#                                             c = 21: K = 6 or 7, smaller group 3: ceil(2^24 / 3) = 5 592 406
#                                             c = 22: K = 6, groups 3 + 3: ceil(2^25 / 3) = 11 184 811
PAIR_ROWS_LOG = 10
PAIR_MIN_PLAIN = {18: 1 << 21, 21: 1 << 24, 22: 1 << 25}
PAIR_MIN_TABLES = {(18, 7): 299594, (18, 8): 1 << 18, (21, 6): 5592406, (21, 7): 5592406, (22, 6): 11184811}


def sort_paths(plan, n, tables=False, chunk_rows=1 << 23):
    """The predicted path of every window group of a call, in schedule order."""
    return [Geometry(plan, n, lo, hi, tables, chunk_rows).path for lo, hi in plan.window_groups(n, tables)]


# c = 21 in the pair form: six windows as two merged windows of three, with an odd entry per part
PAIR21_N = PAIR_MIN_TABLES[(21, 6)]
PAIR21_CASES = [Case(d, c=21, n=PAIR21_N, tables=True, pool=16384) for d in ("exact_edges", "alternating")]
ALL_CASES = (SLOT_CASES + PAIR_CASES + TABLES_CASES + RADIX_CASES + ED_CASES + [NARROW_CASE, INDEXED_CASE] + SHARD_CASES + [BN254_CASE]
             + PAIR21_CASES)


# ---------------------------------------------------------------------------------------------- degenerate pairs in the pair form
# A layout is the roles of m points that share ONE scalar no other point has a digit in common with (a `lone` pool entry of
# count m): every non-zero digit of that scalar is a bucket of exactly these m entries, in point order.  Roles: a capital letter
# is an ordinary point of the set, "-X" its negative, "O" the identity row, "T" the point of order 2 (BLS12-377, calls without
# the endomorphism only).  In the pair form a bucket's entries pair up in that order in round 1 -- an odd one out with nothing,
# pads behind it -- and its round-1 elements, which start at an even element index, pair up in round 2.
DEGENERATE_LAYOUTS = {
    "PPPP": ("P", "P", "P", "P"),            # round 1: two doublings; round 2: a doubling of two equal records
    "PQPQ": ("P", "Q", "P", "Q"),            # round 2: equal sums
    "PQ-P-Q": ("P", "Q", "-P", "-Q"),        # round 2: opposite sums, a cancellation read from records
    "P-PQR": ("P", "-P", "Q", "R"),          # round 1 writes an identity record; round 2 copies B through the second fetch
    "QRP-P": ("Q", "R", "P", "-P"),          # round 2 copies A
    "OPQO": ("O", "P", "Q", "O"),            # identity rows of the point set as first and as second operand
    "PQRSU": ("P", "Q", "R", "S", "U"),      # a fifth element: paired with nothing, then with the sum of a pair of pads
}
TORSION_LAYOUTS = {
    "TTPQ": ("T", "T", "P", "Q"),            # T + T: equal points with y = 0, the identity and not a doubling
    "PTQT": ("P", "T", "Q", "T"),            # generic additions with T; round 2 adds (P + T) + (Q + T)
}
# The pairs of ONE bucket of every layout at logG = 2, as {(round, kind): count} of pair_kinds, written down by hand: m entries
# pair up in order in round 1 (five entries own 8 slots: the fifth is paired with nothing and a pair of pads follows), the
# round-1 elements pair up in round 2.
LAYOUT_PAIRS = {
    "PPPP": {(1, "double"): 2, (2, "double"): 1},
    "PQPQ": {(1, "generic"): 2, (2, "double"): 1},
    "PQ-P-Q": {(1, "generic"): 2, (2, "cancel"): 1},
    "P-PQR": {(1, "cancel"): 1, (1, "generic"): 1, (2, "copy_b"): 1},
    "QRP-P": {(1, "generic"): 1, (1, "cancel"): 1, (2, "copy_a_identity"): 1},
    "OPQO": {(1, "copy_b"): 1, (1, "copy_a_identity"): 1, (2, "generic"): 1},
    "PQRSU": {(1, "generic"): 2, (1, "copy_a_absent"): 1, (1, "zero"): 1, (2, "generic"): 1, (2, "copy_a_identity"): 1},
    "TTPQ": {(1, "cancel"): 1, (1, "generic"): 1, (2, "copy_b"): 1},
    "PTQT": {(1, "generic"): 2, (2, "generic"): 1},
}
# ... and of the bucket that degenerate_pairs_in_parts spreads over two parts, m entries in each: the parts pair up on their own,
# so a layout of four gives the pairs above twice in both rounds; of five, each part leaves its fifth entry paired with nothing,
# the six elements need no pad and round 2 adds (P + Q) + (R + S), U + (P' + Q'), (R' + S') + U'.
LAYOUT_PAIRS_TWO_PARTS = {name: {k: 2 * v for k, v in pairs.items()} for name, pairs in LAYOUT_PAIRS.items() if name != "PQRSU"}
LAYOUT_PAIRS_TWO_PARTS["PQRSU"] = {(1, "generic"): 4, (1, "copy_a_absent"): 2, (2, "generic"): 3}


def check_layout_pairs(dp, kinds):
    """Every bucket of every lone scalar holds exactly the pairs written down for its layout (the planted bucket of
    degenerate_pairs_in_parts: those of two parts)."""
    planted = getattr(dp, "planted", {})
    for j, (name, _) in enumerate(dp.groups):
        assert kinds[j], name
        for l, cnt in kinds[j]:
            cnt = dict(cnt)
            parts = cnt.pop("parts")
            two = planted.get(j) == l
            assert parts == (2 if two else 1), (name, l, parts)
            assert cnt == (LAYOUT_PAIRS_TWO_PARTS if two else LAYOUT_PAIRS)[name], (name, l, cnt)
        assert j not in planted or planted[j] in [l for l, _ in kinds[j]]


class DegeneratePairs:
    """cr: the Crafted input; groups: [(layout name, [point index of every role, ascending])]; edits: [(point index, source
    point index or None, sign, torsion?)] -- row dst becomes sign * row src, the identity (src None) or T."""

    def __init__(self, cr, groups, layouts):
        self.cr, self.groups, self.layouts = cr, groups, layouts
        self.edits = []
        for name, pos in groups:
            first = {}
            for role, at in zip(layouts[name], pos):
                letter = role.lstrip("-")
                if letter == "O":
                    self.edits.append((at, None, 1, False))
                elif letter == "T":
                    self.edits.append((at, None, 1, True))
                elif letter in first:
                    self.edits.append((at, first[letter], -1 if role[0] == "-" else 1, False))
                else:
                    assert role[0] != "-"
                    first[letter] = at

    def values(self, logs, q):
        """{point index: (discrete log, torsion bit)} of every point of a group, after the edits; logs: index -> a_i."""
        out = {at: (logs(at) % q, 0) for _, pos in self.groups for at in pos}
        for at, src, sign, tors in self.edits:
            out[at] = (0, 1) if tors else (0, 0) if src is None else (sign * logs(src) % q, 0)
        return out


def _lone_buckets_ok(cr, n_lone, bucket_sets, planted=None):
    """No bucket of a lone scalar is shared: not with another lone scalar, not with a second digit of the same one, not with any
    other pool entry that has points (craft keeps the uniform fill out, not the classes).  planted: {lone row: (magnitude, windows)}
    -- the one bucket a row fills on purpose from several windows of a merged window; its bin holds no other digit of a lone row."""
    mags = np.abs(cr.digits)
    live = cr.counts > 0
    for lo, hi in bucket_sets:
        lone = mags[:n_lone, :, lo:hi]
        vals = lone[lone > 0]
        uniq, cnt = np.unique(vals, return_counts=True)
        want = {}
        for row, (mag, windows) in (planted or {}).items():
            k_in = [k for k in windows if lo <= k < hi]
            if k_in:
                want[mag] = len(k_in)
                fb = cr.fb[lo]
                others = lone[row][lone[row] != mag]
                if (((others[others > 0] - 1) >> fb) == ((mag - 1) >> fb)).any():
                    return False
        if any(int(c) != want.get(int(u), 1) for u, c in zip(uniq, cnt)):
            return False
        rest = mags[n_lone:, :, lo:hi][live[n_lone:]]
        if np.isin(rest, uniq).any():
            return False
    if planted:      # no stray digit of another lone row in a planted bin either
        for lo, hi in bucket_sets:
            fb = cr.fb[lo]
            bins = {(mag - 1) >> fb for mag, windows in planted.values() if any(lo <= k < hi for k in windows)}
            lone = mags[:n_lone, :, lo:hi]
            stray = (lone > 0) & np.isin((lone - 1) >> fb, list(bins)) & ~np.isin(lone, [m for m, _ in planted.values()])
            if stray.any():
                return False
    return True


def degenerate_pairs(plan, n, seed=21, pool=4096, reps=2, tables=False, layouts=None):
    """Every layout `reps` times among uniform fill: one lone pool entry per group, its points anywhere in the point order."""
    layouts = DEGENERATE_LAYOUTS if layouts is None else layouts
    names = [name for _ in range(reps) for name in layouts]
    classes = [Class(1, [], counts=[len(layouts[name])], lone=True) for name in names]
    bucket_sets = plan.window_groups(n, True) if tables else [(k, k + 1) for k in range(plan.K)]
    for attempt in range(32):
        # (craft keeps the fill out of the lone scalars' buckets, not the lone scalars out of each other's: draw until they are)
        cr = craft("degenerate_pairs", plan, n, classes, seed + 1000 * attempt, pool, tables)
        if _lone_buckets_ok(cr, len(names), bucket_sets):
            break
    else:
        raise AssertionError("no draw without a shared bucket among the lone scalars")
    groups = [(name, np.nonzero(cr.order == j)[0].tolist()) for j, name in enumerate(names)]
    assert all(len(pos) == len(layouts[name]) for name, pos in groups)
    return DegeneratePairs(cr, groups, layouts)


HEAVY_WINDOWS = (1, 4)      # the digit windows of the merged window in which a lone scalar of degenerate_pairs_in_parts has its bucket


def degenerate_pairs_in_parts(plan, n, seed=22, pool=4096, reps=2, layouts=None):
    """The layouts inside a MULTI-PART bin of a merged window (window tables, one group of all K windows).  A heavy class of 256
    pool entries has every digit -- all K windows, both halves -- in one bin b, over the lower half of its buckets: 2 K records
    per point, 2.5 part_len records in all, so the bin is cut into three parts, the cuts falling in windows 2 and 5 (a bin's
    records are ordered by digit window, then point, then half).  Every lone scalar has one bucket of the upper half of bin b as
    its digit in window 1 AND in window 4 (first half): the merged bucket holds the m entries of window 1 in part 0 and the m
    entries of window 4, which read the rows 2^(3c) further up the tables, in part 1.  The parts pair up on their own: a bucket of
    five entries leaves its fifth paired with nothing at the end of BOTH parts, and part 1 starts its pairs at part_pair_off and
    its elements at the sub row of k_part_scan.  pair_kinds walks exactly that."""
    layouts = DEGENERATE_LAYOUTS if layouts is None else layouts
    K, c = plan.K, plan.c
    assert plan.halves == 2 and plan.window_groups(n, True) == [(0, K)] and max(HEAVY_WINDOWS) < K - 1
    window, b, fb, part_len = _target(plan, n, 0, None, True)
    NB = 1 << fb
    names = [name for _ in range(reps) for name in layouts]
    assert len(names) <= NB // 2
    classes, planted = [], {}
    for j, name in enumerate(names):
        off = NB // 2 + j
        classes.append(Class(1, [Plant(k, b, [off]) for k in HEAVY_WINDOWS], counts=[len(layouts[name])], lone=True))
        planted[j] = ((b << fb) + off + 1, HEAVY_WINDOWS)
    m = 256
    heavy_points = -(-(5 * part_len // 2) // (2 * K))
    plants = [Plant(k, b, (np.arange(m) * 5 + 3 * k + h) % (NB // 2), half=h) for k in range(K) for h in range(2)]
    classes.append(Class(m, plants, counts=split_counts(heavy_points, m)))
    for attempt in range(32):
        cr = craft("degenerate_pairs_in_parts", plan, n, classes, seed + 1000 * attempt, pool, True)
        if _lone_buckets_ok(cr, len(names), [(0, K)], planted):
            break
    else:
        raise AssertionError("no draw without a shared bucket among the lone scalars")
    assert 2 * part_len < cr.bins[(0, b)] <= 3 * part_len
    groups = [(name, np.nonzero(cr.order == j)[0].tolist()) for j, name in enumerate(names)]
    dp = DegeneratePairs(cr, groups, layouts)
    dp.planted = {j: mag for j, (mag, _) in planted.items()}
    return dp


ABSENT = None


def combine(A, B, q):
    """(kind, sum) of one pair of the tree as k_batch_add classifies it (ba_denominator, batch_add.h); an operand is ABSENT (an
    empty slot) or (l, t) = l G + t T with T of order 2, (0, 0) the identity."""
    inf_a, inf_b = A is ABSENT or A == (0, 0), B is ABSENT or B == (0, 0)
    if inf_a and inf_b:
        return "zero", (0, 0)
    if inf_b:
        return ("copy_a_absent" if B is ABSENT else "copy_a_identity"), A
    if inf_a:
        return "copy_b", B
    if A == B:                                   # equal points: a doubling unless y = 0, which only T has (2 l = 0 mod q: l = 0)
        return ("cancel", (0, 0)) if A == (0, 1) else ("double", (2 * A[0] % q, 0))
    if A[1] == B[1] and (A[0] + B[0]) % q == 0:  # opposite points (-T = T)
        return "cancel", (0, 0)
    return "generic", ((A[0] + B[0]) % q, A[1] ^ B[1])


def _bin_record_index(cr, lo, hi, fb, b):
    """The records of bin b of the (merged) window [lo, hi) in record order -- by digit window, point, half -- as sorted linear
    indices ((window - lo) * n + point) * halves + half."""
    stack = np.stack([np.abs(cr.digits[:, :, k])[cr.order] for k in range(lo, hi)])
    return np.flatnonzero(((stack > 0) & (((stack - 1) >> fb) == b)).ravel())


def pair_kinds(dp, values, logG, glv=True):
    """Walks the buckets of the lone scalars of `dp` the way the pair form does and counts the pairs of every kind:
    {group index: [Counter((round, kind)) per bucket, ascending by bucket]}.  A bucket of a lone scalar holds entries of its group
    alone (asserted), ordered by digit window (window tables), point, half; entry = sign * lambda^half * 2^(c (window - first of the
    group)) * the point.  A bin of more than part_len records is cut into parts of part_len records (sort_kernels.h, "Parts of heavy
    bins"): round 1 pairs a bucket's entries in order INSIDE each part, the odd one out of a part with nothing, and fills up to
    roundup(2 * elements, 2^logG) / 2 elements with pairs of pads; round 2 pairs the elements."""
    from collections import Counter

    cr, pl = dp.cr, dp.cr.plan
    q, lam, c, n, H = pl.cv.q, pl.cv.B.lam, pl.c, dp.cr.n, dp.cr.plan.halves
    groups = pl.window_groups(cr.n, True) if cr.tables else [(k, k + 1) for k in range(pl.K)]
    hists = cr.stats()[0]
    mags = np.abs(cr.digits)
    live = cr.counts > 0
    bin_index = {}
    out = {}
    for j, (name, pos) in enumerate(dp.groups):
        per_bucket = []
        for gi, (lo, hi) in enumerate(groups):
            for l in sorted({int(m) for m in mags[j, :, lo:hi].ravel() if m}):
                owners = np.argwhere((mags[:, :, lo:hi] == l) & live[:, None, None])
                assert {int(o[0]) for o in owners} == {j}, (name, l, owners)       # no other scalar touches the bucket
                hist = hists[gi] if cr.tables else hists[lo]
                fb, part_len = cr.fb[lo], cr.part_len[lo]
                b = (l - 1) >> fb
                multi = int(hist[1 + (b << fb):1 + ((b + 1) << fb)].sum()) > part_len
                if multi and (lo, b) not in bin_index:
                    bin_index[(lo, b)] = _bin_record_index(cr, lo, hi, fb, b)
                entries = []
                for _, h, kk in owners:
                    d = int(cr.digits[j, h, lo + kk])
                    w = (-1 if d < 0 else 1) * (lam if h else 1) * (1 << (c * int(kk)))
                    for at in pos:
                        v = values[at]
                        assert not (v[1] and (glv or kk)), "T only where a scalar's digits are not split and the tables are not used"
                        key = (int(kk) * n + at) * H + int(h)
                        part = int(np.searchsorted(bin_index[(lo, b)], key)) // part_len if multi else 0
                        entries.append((key, part, (v[0] * w % q, v[1])))
                entries.sort()
                assert len(entries) == int(hist[l])
                cnt = Counter()
                elements = []
                for part in sorted({p for _, p, _ in entries}):
                    mine = [v for _, p, v in entries if p == part]
                    for e in range(0, len(mine), 2):
                        kind, s = combine(mine[e], mine[e + 1] if e + 1 < len(mine) else ABSENT, q)
                        cnt[(1, kind)] += 1
                        elements.append(s)
                G = 1 << logG
                for _ in range((-2 * len(elements) % G) // 2):
                    cnt[(1, "zero")] += 1
                    elements.append((0, 0))
                for e in range(0, len(elements), 2):
                    cnt[(2, combine(elements[e], elements[e + 1], q)[0])] += 1
                cnt["parts"] = len({p for _, p, _ in entries})
                per_bucket.append((l, cnt))
        out[j] = per_bucket
    return out
