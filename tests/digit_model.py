"""The digit kernels' contract in plain Python integers: scalars -> window words `magnitude | sign << 31`.  No GPU, no fixtures.

Every MSM starts in one of the digit kernels (k_digits, k_te_digits, k_digits_narrow<W>, k_te_digits_narrow<W> and their _batch
forms: msm_kernels.h, te_kernels.h, narrow_kernels.h).  This module restates what they must write, for tests/test_gpu_digits.py
to compare with word for word through MsmContext.test_digits:

  decoding   32-byte scalars are reduced mod q when >= q (flag: refused under msm_opts.strict).  Narrow values are unsigned or
             two's complement integers of their width; width 32 holds field elements, a negative value as q - |v| (every stored
             value from 2^129 up is read that way).  Range rule: |v| < 2^bits, or |v| = 2^bits for a negative value; a value
             outside it becomes 0 and fails the call with MSM_ERR_SCALAR.
  GLV        oracle.msm_oracle.glv_decompose (pinned to the reference by tests/test_oracle_kat.py), never restated here.
  plan       make_plan (msm_plan.hip): K = ceil((b + 1) / c); the fold -- c >= 18, b + 1 = (K - 1) c + 1, not on the Edwards
             curve -- takes one window off and makes the top one c + 1 bits wide; the bucket-range shard g of G keeps the bucket
             indices l - 1 in cut(span, g, G), span = 2^(c-1) for a recoded window, 2^c for a folded top window, 2^(bits left)
             for a short one.
  recoding   window k takes c bits plus the carry; l > L = 2^(c-1) becomes 2 L - l with a carry; the folded top window takes
             c + 1 bits and is not recoded (above 2 L: clamped, MSM_ERR_INTERNAL); sign = carry XOR the value's sign; magnitude 0
             is the word 0; the endomorphism entry is 0 under no_glv and narrow; entries outside the shard's range are 0.

Layout: window k is one row -- on the Weierstrass curves 2 n words (entry 2 i = first half of scalar i, 2 i + 1 = second half),
on Ed-on-BLS12-377 n words.  tests/test_digit_model.py checks all of this against the oracle and tests/crafted_digits.py.
"""
import os
import sys

import numpy as np

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from degenerate_inputs import CURVE_TABLE, NAMES  # noqa: E402,F401
from oracle import msm_oracle as O  # noqa: E402

MSM_OK, MSM_ERR_ARG, MSM_ERR_SCALAR, MSM_ERR_INTERNAL = 0, 1, 6, 7   # include/msm_hip.h
SIGN = 1 << 31
WIDTHS = (1, 2, 4, 8, 16, 32)
TWO256 = 1 << 256


# ---------------------------------------------------------------------------------------------- the plan

def width_full_bits(width, signed):
    """Magnitude bits a narrow width holds (narrow_format, msm_narrow.hip): 128 at most."""
    return 128 if width == 32 else 8 * width - (1 if signed else 0)


class Plan:
    """make_plan for (curve, c, no_glv | narrow_bits, bucket shard (g, G)); use plan(), which returns None where it refuses."""

    def __init__(self, curve, c, no_glv=False, narrow_bits=0, shard=None):
        cv = CURVE_TABLE[curve]
        self.curve, self.cv, self.c, self.te, self.narrow_bits, self.shard = curve, cv, c, cv.te, narrow_bits, shard
        self.no_glv = (not cv.te) and bool(narrow_bits or no_glv)
        self.glv = not cv.te and not self.no_glv               # two halves from the endomorphism split
        b = narrow_bits if narrow_bits else 251 if cv.te else cv.q.bit_length() if self.no_glv else cv.glv.max_bits
        self.bits = b + 1
        self.K = -(-self.bits // c)
        self.fold = (not cv.te) and c >= 18 and self.K > 1 and self.bits - (self.K - 1) * c == 1
        if self.fold:
            self.K -= 1
        self.L_log = c if self.fold else c - 1
        self.per_point = 1 if cv.te else 2
        self.top_bits = c if self.fold else min(c - 1, self.bits - (self.K - 1) * c)
        self.ranges = None
        if shard is not None:
            g, G = shard
            low = self.cut((1 << (c - 1)) if self.K > 1 else 1 << max(0, self.top_bits), g, G)
            self.ranges = [low] * (self.K - 1) + [self.cut(1 << max(0, self.top_bits), g, G)]

    def cut(self, span, g, G):
        """Bucket indices [lo, hi) of part g of G of a window whose digits cover `span` buckets; the last part runs to the end."""
        return span * g // G, ((1 << self.L_log) if g + 1 == G else span * (g + 1) // G)

    def kind(self):
        """'folded', 'short' or 'full': what the top window is."""
        return "folded" if self.fold else "short" if self.bits - (self.K - 1) * self.c < self.c else "full"


def plan(curve, c, no_glv=False, narrow_bits=0, shard=None):
    """The plan, or None where make_plan answers MSM_ERR_ARG."""
    cv = CURVE_TABLE[curve]
    if c < 2 or c > 24:
        return None
    if (not cv.te) and no_glv and not narrow_bits and c < 4:
        return None                                            # keeps K <= 64
    if narrow_bits and (narrow_bits + c) // c > 64:
        return None
    if shard is not None and not 0 <= shard[0] < shard[1]:
        return None
    return Plan(curve, c, no_glv, narrow_bits, shard)


# ---------------------------------------------------------------------------------------------- decoding

def decode_full(raw, q):
    """A 32-byte scalar as stored -> (value mod q, was it >= q)."""
    return raw % q, raw >= q


def decode_narrow(raw, width, bits, signed, q):
    """A narrow scalar as stored (the unsigned integer of its `width` bytes) -> (magnitude, negative, refused).  A refused value
    counts as 0."""
    if width == 32:
        bad = raw >= q
        neg = bool(signed) and raw >= (1 << 129)
        mag = (q - raw) % TWO256 if neg else raw
    else:
        bad = False
        neg = bool(signed) and raw >> (8 * width - 1) == 1
        mag = (1 << (8 * width)) - raw if neg else raw
    if not (mag < (1 << bits) or (neg and mag == (1 << bits))):
        bad = True
    return (0, False, True) if bad else (mag, neg, False)


def encode_narrow(v, width, q):
    """The signed integer v as a narrow scalar is stored: two's complement of the width, or q - |v| for width 32."""
    if width == 32:
        return v if v >= 0 else q + v
    return v % (1 << (8 * width))


# ---------------------------------------------------------------------------------------------- recoding

def recode(mag, neg, pl):
    """K words of one entry (before the shard filter), and whether the folded top window had to be clamped."""
    c, K = pl.c, pl.K
    L = 1 << (c - 1)
    out, carry, clamped = [], 0, False
    for k in range(K):
        top = pl.fold and k == K - 1
        l = ((mag >> (c * k)) & ((1 << (c + 1 if top else c)) - 1)) + carry
        if not top and l > L:
            l, carry = 2 * L - l, 1
        else:
            carry = 0
        if top and l > 2 * L:
            l, clamped = 2 * L, True
        out.append(l | (SIGN if (l and (carry ^ int(neg))) else 0))
    # nothing may be left above the windows: K c >= bits + 1 keeps the carry inside the top window
    assert carry == 0 and (clamped or mag >> (c * K + (1 if pl.fold else 0)) == 0), (mag, c, K)
    return out, clamped


def shard_filter(words, pl):
    if pl.ranges is None:
        return words
    return [w if (w and pl.ranges[k][0] <= (w & ~SIGN) - 1 < pl.ranges[k][1]) else 0 for k, w in enumerate(words)]


def word_value(words, c):
    """sum_k +-l_k 2^(c k) of one entry's words."""
    return sum((-(w & ~SIGN) if w & SIGN else (w & ~SIGN)) << (c * k) for k, w in enumerate(words))


def scalar_entries(raw, pl, fmt=None):
    """One stored scalar -> ([(magnitude, negative)] per entry of the point: 2 on a Weierstrass curve, 1 on the Edwards curve,
    flags).  fmt = (width, bits, signed) for a narrow call.  flags: 'ge_q', 'range'."""
    q = pl.cv.q
    flags = set()
    if fmt is not None:
        mag, neg, bad = decode_narrow(raw, fmt[0], fmt[1], fmt[2], q)
        if bad:
            flags.add("range")
        ent = [(mag, neg)]
    else:
        v, ge = decode_full(raw, q)
        if ge:
            flags.add("ge_q")
        if pl.glv:
            m0, m1, n0, n1 = O.glv_decompose(v, pl.cv.glv)
            ent = [(m0, n0), (m1, n1)]
        else:
            ent = [(v, False)]
    if not pl.te and len(ent) == 1:
        ent.append((0, False))                                  # the endomorphism entry of no_glv and narrow calls
    return ent, flags


def return_code(flags, strict=False):
    """What the real calls make of the error word (check_scalar_flags, msm_pipeline.hip)."""
    if (strict and "ge_q" in flags) or "range" in flags:
        return MSM_ERR_SCALAR
    return MSM_ERR_INTERNAL if "fold" in flags else MSM_OK


def model_words(pl, raws, fmt=None, strict=False):
    """(K, per_point * len(raws)) uint32 words and the return code for the stored scalars `raws` (Python integers)."""
    out = np.zeros((pl.K, pl.per_point * len(raws)), dtype=np.uint32)
    flags = set()
    for i, raw in enumerate(raws):
        ent, f = scalar_entries(raw, pl, fmt)
        flags |= f
        for h, (mag, neg) in enumerate(ent):
            words, clamped = recode(mag, neg, pl)
            if clamped:
                flags.add("fold")
            out[:, pl.per_point * i + h] = shard_filter(words, pl)
    return out, return_code(flags, strict)


# ---------------------------------------------------------------------------------------------- the scalars of the sweep

def patterns(c, K, fold, b):
    """Magnitudes below 2^b that put the recoding's edges into every window: a raw digit of L - 1, L, L + 1 and 2^c - 1 in
    window j, alone and (near both ends) on top of all-ones, so that a carry arrives; a carry that runs through every window;
    a top window that holds only the carry; L and L + 1 in all windows at once."""
    L, top_mask = 1 << (c - 1), (1 << b) - 1
    near_ends = set(range(min(K, 3))) | set(range(max(0, K - 3), K))
    out = [top_mask, top_mask >> 1, (1 << (c * (K - 1))) - 1, 1 << (c * (K - 1)), (1 << (c * (K - 1))) + 1]
    out.append(sum(L << (c * j) for j in range(K)) & top_mask)
    out.append(sum((L + 1) << (c * j) for j in range(K)) & top_mask)
    for j in range(K):
        for d in (L - 1, L, L + 1, (1 << c) - 1):
            out.append((d << (c * j)) & top_mask)
            if j in near_ends and j:
                out.append(((d << (c * j)) | ((1 << (c * j)) - 1)) & top_mask)
    if fold:
        out += [1 << b >> 1, (1 << b >> 1) | ((1 << (c * (K - 1))) - 1)]   # the extra bit of the folded top window, alone and with a carry
    seen, uniq = set(), []
    for v in out:
        if v not in seen:
            seen.add(v)
            uniq.append(v)
    return uniq


def fixed_scalars(cv):
    """(below q, from q up): 0, 1, q - 1 and the endomorphism's lambda with its neighbours; q, q + 1, 2 q + 3, 2^256 - 1 and
    multiples of q up to the last one below 2^256 (55 subtractions on the Edwards curve)."""
    q = cv.q
    low = [0, 1, 2, q - 1, q - 2]
    if not cv.te:
        lam = cv.B.lam
        low += [lam, lam - 1, lam + 1, q - lam, q - lam - 1, q - lam + 1]
    top = (TWO256 - 1) // q
    high = [q, q + 1, 2 * q + 3, TWO256 - 1, top * q, top * q - 1, (top - 1) * q + 5]
    high += [m * q + 7 * m for m in (3, 5, 9, 13, 16, 17, 31, 54, 55) if m * q + 7 * m < TWO256]
    return low, [v for v in dict.fromkeys(high) if v >= q]


def full_scalars(pl, n_random=500, room=None):
    """(scalars below q, scalars from q up) of one full-width configuration: the fixed ones, the patterns of the plan -- on a
    curve with the endomorphism as (+-h0 +- lambda h1) mod q, so that the halves carry them where the decomposition gives them
    back, and as they are --, and n_random from O.prng_ints.  room: at most that many scalars in all (the randoms give way)."""
    cv, q = pl.cv, pl.cv.q
    low, high = fixed_scalars(cv)
    pat = patterns(pl.c, pl.K, pl.fold, pl.bits - 1)
    if pl.glv:
        lam, m = cv.B.lam, len(pat)
        # every pattern as a positive first half beside a short second half (short halves come back from the decomposition as
        # they went in), as a negative one beside a full pattern, and somewhere as a second half
        for i, h0 in enumerate(pat):
            s1 = (1, -1)[i & 1]
            low.append((h0 + s1 * lam * (pat[(7 * i + 3) % m] >> 32)) % q)
            low.append((-h0 - s1 * lam * pat[(5 * i + 1) % m]) % q)
        low += [(lam * h) % q for h in pat[:8]] + [h % q for h in pat[:8]]
    else:
        low += [v for v in pat if v < q]
        high += [v for v in pat if v >= q]
    low, high = list(dict.fromkeys(low)), list(dict.fromkeys(high))
    if room is not None:
        n_random = min(n_random, room - len(low) - len(high))
        assert n_random >= 100, (pl.curve, pl.c, len(low), len(high))
    low += O.prng_ints(f"digits/{pl.curve}/{pl.c}/{int(pl.glv)}", n_random, q)
    return low, high


def narrow_values(pl, width, bits, signed, n_random=150):
    """(accepted, refused) signed integers of one narrow format: 0, +-1, 2^bits - 1, -2^bits (accepted), +2^bits (refused), the
    width's minimum and maximum, the plan's patterns with both signs, and randoms below 2^bits."""
    full = width_full_bits(width, signed)
    lo_w = -(1 << (8 * width - 1)) if signed and width < 32 else 0
    hi_w = (1 << (8 * width - 1)) - 1 if signed and width < 32 else (1 << (8 * width)) - 1 if width < 32 else None
    cand = [0, 1, 2, (1 << bits) - 1, (1 << bits) - 2, 1 << bits, (1 << bits) + 1, 1 << (bits - 1)]
    cand += patterns(pl.c, pl.K, pl.fold, bits)
    cand += O.prng_ints(f"digits/narrow/{width}/{bits}/{int(signed)}/{pl.c}", n_random, 1 << bits)
    if signed:
        cand += [-v for v in cand]
    if width < 32:
        cand += [lo_w, hi_w, lo_w + 1, hi_w - 1]
    else:
        cand += [1 << 128, (1 << 128) + 1, (1 << 129) - 1] + ([-(1 << 128)] if signed else [])
    ok, bad = [], []
    for v in dict.fromkeys(cand):
        if width < 32 and not lo_w <= v <= hi_w:
            continue                                            # the width cannot store it
        (ok if (abs(v) < (1 << bits) or v == -(1 << bits)) else bad).append(v)
    assert bits <= full
    return ok, bad


def stored_extremes_32(cv, signed):
    """Stored 32-byte words of a width-32 call that no signed integer of narrow_values names: q - 1 (-1 when signed), q and
    2^256 - 1 (never scalars), 2^129 (signed: -(q - 2^129), far outside any range).  -> [(stored, refused?)]"""
    q = cv.q
    return [(q - 1, not signed), (q, True), (TWO256 - 1, True), (1 << 129, True), (q - (1 << 128) - 1, True)]


def to_bytes(raws, width):
    """Stored scalars (unsigned integers) -> (len, width) uint8 array, little-endian."""
    return np.frombuffer(b"".join(int(r).to_bytes(width, "little") for r in raws), dtype=np.uint8).reshape(len(raws), width)
