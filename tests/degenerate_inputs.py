"""Degenerate point multisets for every MSM entry point and curve: plain helpers, no fixtures, no GPU.

The tree of an MSM mostly meets two finite points with different x.  The inputs built here make the other cases the rule: runs
of one and the same point (every pair of a run is P + P, then 2P + 2P, ... down the tree), runs that alternate Q, -Q (every
pair cancels), identities at both ends, in a run longer than a wave and sprinkled over the rest, points of even order outside
the prime-order subgroup, and -- for the window tables, whose windows share one set of buckets -- chains P, 2^c P, 2^2c P, ...
whose table rows of DIFFERENT windows are equal or opposite points of one merged bucket.

Every input point is an entry (j, sign, identity?) over a pool of 64 points Q_j = k_j G with known k_j, so the expected value
of any MSM over them is ONE scaling, (sum sign_i s_i k_j(i) mod q) G, whatever n is: expected().  tests/test_degenerate_inputs.py
proves that value equal to the oracle's plain sum at a small n before tests/test_gpu_degenerate_points.py relies on it.
"""
import functools
import os
import sys

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from oracle import msm_oracle as O  # noqa: E402
from test_cycle_curves import CURVES as CYCLE_CURVES  # noqa: E402

POOL = 64
RUN_LENGTHS = (2, 3, 4, 63, 64, 65, 129, 257, 1025)   # across a wave (64) and a 256-lane workgroup, into the descriptor rounds
IDENT = (0, 1, True)                                  # an input entry: (pool index, sign, identity?)
SCALAR_LAYOUTS = ("dbl", "cancel", "generic", "sparse")
# narrow formats of msm_run_narrow: name -> (width in bytes, signed, bits argument, magnitude bits of the values)
NARROW_FORMATS = {"int32_b16": (4, True, 16, 16), "uint64": (8, False, None, 64), "field_b128": (32, True, 128, 128)}


class Curve:
    """One curve of include/msm_hip.h: its id, the oracle's parameters, and the point arithmetic the expected values need."""

    def __init__(self, name, cid, B, te=False):
        self.name, self.cid, self.B, self.te = name, cid, B, te
        self.p, self.q, self.cb = B.p, B.q, B.n_bytes
        self.glv = None if te else O.glv_params(B.q, B.lam)
        self.scalar_bits = 251 if te else self.glv.max_bits    # b of K = ceil((b + 1) / c): GLV halves, or the Edwards order
        self.zero = (0, 1) if te else None                     # the identity as results and expected values carry it

    def scale_g(self, k):
        """k G as an affine result: (x, y), the identity as None (Weierstrass) or (0, 1) (Edwards)."""
        B = self.B
        if self.te:
            return O.te_to_affine(O.te_scale(k % B.q, O.te_from_affine((B.gx, B.gy), B), B), B)
        return O.aff_scale(k % B.q, (B.gx, B.gy), B.p)

    def add(self, P, Q):
        B = self.B
        if self.te:
            return O.te_to_affine(O.te_add(O.te_from_affine(P, B), O.te_from_affine(Q, B), B), B)
        return O.aff_add(P, Q, B.p)

    def scale(self, s, P):
        B = self.B
        if self.te:
            return O.te_to_affine(O.te_scale(s, O.te_from_affine(P, B), B), B)
        return O.aff_scale(s, P, B.p)

    def neg(self, P):
        if self.te:
            return ((-P[0]) % self.p, P[1])
        return O.aff_neg(P, self.p)

    def naive_msm(self, scalars, points):
        """The oracle's own sum over the same points and scalars (Edwards: its msmBasic restatement)."""
        if self.te:
            return O.msm_basic_te(list(scalars), list(points), self.B)
        return O.msm_naive_affine(scalars, points, self.B)

    def plan_k(self, c):
        """Windows of the plain plan under c (make_plan): ceil((b + 1) / c), one less where the carry bit folds into the top."""
        bits = self.scalar_bits + 1
        K = -(-bits // c)
        if not self.te and c >= 18 and K > 1 and bits - (K - 1) * c == 1:
            K -= 1
        return K

    def wire(self, points):
        """x || y little-endian per point; the identity as wire zeros (Weierstrass) or (0, 1) (Edwards)."""
        cb = self.cb
        return b"".join(bytes(2 * cb) if P is None else P[0].to_bytes(cb, "little") + P[1].to_bytes(cb, "little") for P in points)


CURVE_TABLE = {
    "bls377": Curve("bls377", 0, O.BLS12_377),
    "ed377": Curve("ed377", 1, O.ED_ON_BLS12_377, te=True),
    "bls381": Curve("bls381", 2, O.BLS12_381),
    "pallas": Curve("pallas", 3, O.PALLAS),
}
for _name, _entry in CYCLE_CURVES.items():
    CURVE_TABLE[_name] = Curve(_name, _entry[0], _entry[1])
NAMES = ("bls377", "bls381", "pallas", "ed377", "bn254", "grumpkin", "vesta")
assert set(NAMES) == set(CURVE_TABLE)


@functools.lru_cache(maxsize=None)
def pool(name):
    """(points, logs): 64 points Q_j = k_j G of the curve."""
    cv = CURVE_TABLE[name]
    if cv.te:
        return O.random_points_ed377(f"degenerate/{name}", POOL)
    return O.random_points_bls377(f"degenerate/{name}", POOL, cv.B)


def point_of(cv, entry):
    j, sign, ident = entry
    if ident:
        return cv.zero
    P = pool(cv.name)[0][j]
    return P if sign > 0 else cv.neg(P)


def points_of(cv, entries):
    memo = {}
    for e in set(entries):
        memo[e] = point_of(cv, e)
    return [memo[e] for e in entries]


def expected(cv, entries, scalars):
    """(sum sign_i s_i k_j(i) mod q) G.  The scalars are integers of either sign (narrow values enter signed)."""
    logs = pool(cv.name)[1]
    return cv.scale_g(sum(sign * s * logs[j] for (j, sign, ident), s in zip(entries, scalars) if not ident) % cv.q)


# ---------------------------------------------------------------------------------------------- the point layout

class Layout:
    """entries: the n input entries; runs: (first index, length, "eq" | "alt") of every run of one point resp. of Q, -Q, Q, ...;
    ident_run: (first index, length) of the run of identities."""

    def __init__(self, entries, runs, ident_run):
        self.entries, self.runs, self.ident_run, self.n = entries, runs, ident_run, len(entries)

    def longest_eq_run(self):
        return max((r for r in self.runs if r[2] == "eq"), key=lambda r: r[1])


def run_lengths(n):
    """n >= 5000: all nine; n = 1000: they stop at 129; a small n (the CPU check): 2 ... 9."""
    if n >= 5000:
        return RUN_LENGTHS
    if n >= 1000:
        return RUN_LENGTHS[:7]
    return (2, 3, 4, 5, 9)


@functools.lru_cache(maxsize=None)
def layout(n):
    """One point layout, shared by all scalar layouts (msm_run_batch has one point set for all its elements): the identity at
    index 0; from index 1 the runs of one point, then the runs alternating Q, -Q, pool points between them; a run of identities
    (70, longer than a wave); the remainder pool points with every 8th an identity; the identity at index n - 1."""
    lengths = run_lengths(n)
    entries, runs, nxt = [IDENT], [], 0
    for kind in ("eq", "alt"):
        for length in lengths:
            runs.append((len(entries), length, kind))
            entries += [(nxt % POOL, -1 if (kind == "alt" and t % 2) else 1, False) for t in range(length)]
            entries.append(((nxt + 1) % POOL, 1, False))      # another point between two runs
            nxt += 2
    ident_run = (len(entries), 70 if n >= 1000 else 7)
    entries += [IDENT] * ident_run[1]
    first = len(entries)
    assert first + 16 <= n, "n is too small for the runs"
    for i in range(first, n):
        if (i - first) % 8 == 7:
            entries.append(IDENT)
        else:
            entries.append((nxt % POOL, 1, False))
            nxt += 1
    entries[n - 1] = IDENT
    return Layout(tuple(entries), tuple(runs), ident_run)


def scalars(cv, lay, kind):
    """n integers in [0, q) over layout `lay`.
    dbl: one scalar per run (every pair inside a run of one point is P + P, then 2P + 2P ...; on the alternating runs every pair
    cancels); cancel: inside the runs of one point s, q - s alternate (an even run leaves an identity bucket for the finish and
    the reduction, an odd one leaves one point); generic: independent scalars, equal points meet where digits collide;
    sparse: dbl with 90 % of the scalars zero.  Outside the runs all four are independent scalars (identities included)."""
    assert kind in SCALAR_LAYOUTS
    n, q = lay.n, cv.q
    out = O.prng_ints(f"degenerate/{cv.name}/{n}/generic", n, q)
    if kind == "generic":
        return out
    per_run = [v or 1 for v in O.prng_ints(f"degenerate/{cv.name}/{n}/run", len(lay.runs), q)]
    for r, (start, length, rk) in enumerate(lay.runs):
        for t in range(length):
            s = per_run[r]
            if kind == "cancel" and rk == "eq" and t % 2:
                s = q - s
            out[start + t] = s
    if kind == "sparse":
        keep = O.prng_ints(f"degenerate/{cv.name}/{n}/keep", n, 10)
        out = [s if k == 0 else 0 for s, k in zip(out, keep)]
    return out


def narrow_values(cv, lay, kind, fmt):
    """The scalar layouts restated on narrow values (signed integers): dbl = one value per run, cancel = v, -v inside the runs
    of one point (signed formats only: an unsigned format has no -v)."""
    _, signed, _, mag = NARROW_FORMATS[fmt]
    assert kind in SCALAR_LAYOUTS and (signed or kind != "cancel")
    n = lay.n
    raw = O.prng_ints(f"degenerate/{cv.name}/{n}/{fmt}/generic", n, 1 << (mag + (1 if signed else 0)))
    out = [v - (1 << mag) for v in raw] if signed else raw
    if kind == "generic":
        return out
    per_run = [v + 1 for v in O.prng_ints(f"degenerate/{cv.name}/{n}/{fmt}/run", len(lay.runs), (1 << mag) - 1)]
    for r, (start, length, rk) in enumerate(lay.runs):
        for t in range(length):
            out[start + t] = -per_run[r] if (kind == "cancel" and rk == "eq" and t % 2) else per_run[r]
    if kind == "sparse":
        keep = O.prng_ints(f"degenerate/{cv.name}/{n}/keep", n, 10)
        out = [v if k == 0 else 0 for v, k in zip(out, keep)]
    return out


# ---------------------------------------------------------------------------------------------- chains for the window tables

def chain_scalar_is_whole(cv, s):
    """The scalar reaches the digits as it is: GLV leaves it in the first half (the Edwards path: it is below q, not reduced)."""
    if cv.te:
        return 0 <= s < cv.q
    return O.glv_decompose(s, cv.glv) == (s, 0, False, False)


@functools.lru_cache(maxsize=None)
def chain(name, c, pad_to=0):
    """Points P_0 = Q, P_(i+1) = 2^c P_i (i < K - 1), then the same chain with P_(i+1) = -2^c P_i, computed from the logs; scalars
    s_i = d 2^(c (K - 1 - i)) with one digit 0 < d < 2^(c-1), the same for both chains.  Row i of table k is 2^(c k) P_i, so on
    window tables window K - 1 - i of point i addresses 2^(c (K - 1)) Q for every i of the first chain -- K equal points in the
    merged bucket d, adjacent in point order -- and +-2^(c (K - 1)) Q' alternating on the second: opposite points.  No plain plan
    puts the windows of one scalar into one bucket.  K starts at the plan's and is shortened until every s_i stays whole
    (chain_scalar_is_whole); at least two links must remain.  pad_to: pool points with zero scalars behind the chains (window
    tables need 4096 points; a zero scalar adds no entry, the chain's stay adjacent).
    Returns (points, scalars, expected, K, d)."""
    cv = CURVE_TABLE[name]
    q = cv.q
    pts, logs = pool(name)
    d = O.prng_ints(f"degenerate/{name}/chain/{c}", 1, (1 << (c - 1)) - 1)[0] + 1
    K = cv.plan_k(c)
    while K >= 2 and not all(chain_scalar_is_whole(cv, d << (c * (K - 1 - i))) for i in range(K)):
        K -= 1
    assert K >= 2, f"{name}: no chain of two links under c = {c}"
    sc = [d << (c * (K - 1 - i)) for i in range(K)]
    assert all(chain_scalar_is_whole(cv, s) for s in sc)
    assert all((s >> (c * (K - 1 - i))) == d and s & ((1 << (c * (K - 1 - i))) - 1) == 0 for i, s in enumerate(sc))
    log_a = [logs[5] * pow(2, c * i, q) % q for i in range(K)]
    log_b = [logs[6] * pow(-(1 << c), i, q) % q for i in range(K)]
    all_logs = log_a + log_b
    points = [pts[5]] + [cv.scale_g(k) for k in log_a[1:]] + [pts[6]] + [cv.scale_g(k) for k in log_b[1:]]
    all_sc = sc + sc
    total = sum(s * k for s, k in zip(all_sc, all_logs)) % q
    n_pad = max(0, pad_to - len(points))
    points += [pts[i % POOL] for i in range(n_pad)]
    all_sc += [0] * n_pad
    return points, all_sc, cv.scale_g(total), K, d


# ---------------------------------------------------------------------------------------------- points outside the subgroup

def torsion_points(cv):
    """(point, order) of the curve points of small even order the layouts plant: BLS12-377 (p - 1, 0) of order 2 -- doubling it
    has denominator 2 y = 0 --; Ed-on-BLS12-377 (0, p - 1) of order 2 and (+-i, 0) of order 4."""
    p = cv.p
    if cv.name == "bls377":
        assert O.aff_is_on_curve((p - 1, 0), cv.B)
        return [((p - 1, 0), 2)]
    assert cv.name == "ed377"
    i = O.sqrt_mod(p - 1, p)
    out = [((0, p - 1), 2), ((i, 0), 4), ((p - i, 0), 4)]
    for T, order in out:
        assert O.te_is_on_curve(O.te_from_affine(T, cv.B), cv.B)
        assert cv.scale(order, T) == (0, 1) and cv.scale(order // 2, T) != (0, 1)
    return out


def torsion(name, n, narrow_fmt=None):
    """n pool points with independent scalars and torsion points planted at 5 places, two of them adjacent under one scalar.
    Expected: the generic part plus (sum s mod order) T per torsion point.  Only for paths without the endomorphism: with GLV,
    phi(T) != lambda T and the sum is not defined.  narrow_fmt: signed values of that format instead of scalars below q.
    Returns (points, scalars, expected)."""
    cv = CURVE_TABLE[name]
    tors = torsion_points(cv)
    entries = [(i % POOL, 1, False) for i in range(n)]
    if narrow_fmt is None:
        sc = O.prng_ints(f"degenerate/{name}/torsion/{n}", n, cv.q)     # below q: the Edwards path reduces nothing, s mod 4 stays
    else:
        _, signed, _, mag = NARROW_FORMATS[narrow_fmt]
        raw = O.prng_ints(f"degenerate/{name}/torsion/{n}/{narrow_fmt}", n, 1 << (mag + (1 if signed else 0)))
        sc = [v - (1 << mag) for v in raw] if signed else raw
    places = [3, n // 3, n // 3 + 1, n // 2 + 7, n - 2]
    sc[n // 3 + 1] = sc[n // 3]
    # every torsion point of the curve occurs; places 1 and 2 are the adjacent pair: the same point, the same scalar
    which = [tors[t % len(tors)] for t in (0, 1, 1, 2, 0)]
    points = points_of(cv, entries)
    acc = None
    for at, (T, order) in zip(places, which):
        points[at] = T
        entries[at] = IDENT                                            # (left out of the discrete-log part)
        part = cv.scale(sc[at] % order, T)
        acc = part if acc is None else cv.add(acc, part)
    exp = cv.add(expected(cv, entries, sc), acc)
    return points, sc, exp
