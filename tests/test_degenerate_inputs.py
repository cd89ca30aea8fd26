"""The references of tests/degenerate_inputs.py checked before any GPU sees them (`-m "not gpu"`).

For every curve, at layout(97) (runs of 2 ... 9 points) and under every scalar layout, for the chains of the window tables and
for the points outside the subgroup: the discrete-log expected value, one scaling of G, equals the oracle's plain sum over the
same points and scalars (msm_naive_affine; msm_basic_te on the Edwards curve).  And the precondition of the chains holds: every
chain scalar passes the GLV decomposition whole, under the windows the GPU tests build tables for.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degenerate_inputs as D  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

N = 97


def test_layout_has_every_degenerate_shape():
    for n, lengths in ((N, (2, 3, 4, 5, 9)), (1000, D.RUN_LENGTHS[:7]), (5000, D.RUN_LENGTHS)):
        lay = D.layout(n)
        e = lay.entries
        assert lay.n == len(e) == n and e[0] == D.IDENT and e[n - 1] == D.IDENT and lay.runs[0][0] == 1
        assert [r[1] for r in lay.runs] == list(lengths) * 2
        for start, length, kind in lay.runs:
            run = e[start : start + length]
            assert len({j for j, _, _ in run}) == 1 and not any(ident for _, _, ident in run)
            assert [s for _, s, _ in run] == [(-1 if (kind == "alt" and t % 2) else 1) for t in range(length)]
            assert e[start - 1][0] != run[0][0] or e[start - 1][2]          # another point (or the identity) on either side
            assert e[start + length][0] != run[0][0]
        a, m = lay.ident_run
        assert m == (70 if n >= 1000 else 7) and all(x == D.IDENT for x in e[a : a + m])
        rest = e[a + m : n - 1]
        assert sum(1 for x in rest if x[2]) == len(rest) // 8 and all(x[2] == (i % 8 == 7) for i, x in enumerate(rest))
    assert D.layout(5000).longest_eq_run()[1] == 1025 and D.layout(1000).longest_eq_run()[1] == 129


@pytest.mark.parametrize("kind", D.SCALAR_LAYOUTS)
@pytest.mark.parametrize("name", D.NAMES)
def test_discrete_log_value_is_the_naive_sum(name, kind):
    cv = D.CURVE_TABLE[name]
    lay = D.layout(N)
    sc = D.scalars(cv, lay, kind)
    assert all(0 <= s < cv.q for s in sc)
    if kind == "dbl":
        for start, length, _ in lay.runs:
            assert len(set(sc[start : start + length])) == 1
    if kind == "cancel":
        for start, length, rk in lay.runs:
            assert all((sc[start + t] + sc[start + t + 1]) % cv.q == 0 for t in range(length - 1)) == (rk == "eq")
    if kind == "sparse":
        assert sum(1 for s in sc if s == 0) > N // 2
    exp = D.expected(cv, lay.entries, sc)
    assert exp == cv.naive_msm(sc, D.points_of(cv, lay.entries))
    if kind == "generic":
        assert exp != cv.zero


def signed_naive_sum(cv, values, points):
    """sum v_i P_i term by term with the curve's own scaling and addition: |v| P, negated where v < 0 (equal terms scaled once)."""
    memo, acc = {}, cv.zero
    for v, P in zip(values, points):
        if v == 0 or P == cv.zero:
            continue
        if (v, P) not in memo:
            term = cv.scale(abs(v), P)
            memo[v, P] = term if v > 0 else cv.neg(term)
        acc = cv.add(acc, memo[v, P])
    return acc


@pytest.mark.parametrize("fmt", sorted(D.NARROW_FORMATS))
@pytest.mark.parametrize("name", D.NAMES)
def test_narrow_values_fit_their_format_and_sum_to_the_same_value(name, fmt):
    cv = D.CURVE_TABLE[name]
    lay = D.layout(N)
    _, signed, _, mag = D.NARROW_FORMATS[fmt]
    for kind in D.SCALAR_LAYOUTS:
        if kind == "cancel" and not signed:
            continue
        vals = D.narrow_values(cv, lay, kind, fmt)
        assert all((-(1 << mag) if signed else 0) <= v < (1 << mag) for v in vals)
        if kind == "generic" and signed:
            assert min(vals) < 0 < max(vals)
        assert D.expected(cv, lay.entries, vals) == signed_naive_sum(cv, vals, D.points_of(cv, lay.entries)), kind


def table_windows(cv):
    return (14, 17) if cv.te else (16, 18)


@pytest.mark.parametrize("name", D.NAMES)
def test_chain_precondition_and_value(name):
    cv = D.CURVE_TABLE[name]
    for c in table_windows(cv) + (13,):
        points, sc, exp, K, d = D.chain(name, c)
        assert 2 <= K <= cv.plan_k(c) and 0 < d < (1 << (c - 1)) and len(points) == len(sc) == 2 * K
        for i in range(K):
            s = sc[i]
            assert s == sc[K + i] == d << (c * (K - 1 - i))
            if not cv.te:
                assert O.glv_decompose(s, cv.glv) == (s, 0, False, False), (c, i)
            assert s < cv.q
            # the one non-zero signed digit is d, in window K - 1 - i
            digits = O.signed_digits(s, c, cv.plan_k(c) + 1)
            assert [(l, neg) for l, neg in digits if l] == [(d, False)] and digits[K - 1 - i] == (d, False)
        # the rows window K - 1 - i of point i addresses on tables: equal on the first chain, +- alternating on the second
        rows_a = [cv.scale(1 << (c * (K - 1 - i)), points[i]) for i in range(K)]
        rows_b = [cv.scale(1 << (c * (K - 1 - i)), points[K + i]) for i in range(K)]
        assert len(set(rows_a)) == 1 and rows_a[0] != cv.zero
        assert all(rows_b[i] == (rows_b[0] if i % 2 == 0 else cv.neg(rows_b[0])) for i in range(K)) and rows_b[1] != rows_b[0]
        assert exp == cv.naive_msm(sc, points)
        padded = D.chain(name, c, 40)
        assert len(padded[0]) == 40 and padded[1][2 * K :] == [0] * (40 - 2 * K) and padded[2] == exp and padded[0][: 2 * K] == points


@pytest.mark.parametrize("name", ["bls377", "ed377"])
def test_torsion_value_is_the_naive_sum(name):
    cv = D.CURVE_TABLE[name]
    for fmt in (None, "int32_b16", "uint64"):
        points, sc, exp = D.torsion(name, 40, fmt)
        tors = [T for T, _ in D.torsion_points(cv)]
        at = [i for i, P in enumerate(points) if P in tors]
        assert {points[i] for i in at} == set(tors)                     # every torsion point of the curve is planted
        assert len(at) == 5 and any(b == a + 1 and points[a] == points[b] and sc[a] == sc[b] for a, b in zip(at, at[1:]))
        if fmt is None:
            assert exp == cv.naive_msm(sc, points)
        # every term on its own, with its sign (narrow values may be negative), summed by the curve's own addition
        assert signed_naive_sum(cv, sc, points) == exp, fmt
    if name == "bls377":
        T = tors[0]
        assert O.aff_double(T, cv.p) is None and O.aff_scale(cv.q, T, cv.p) == T      # order 2: outside the subgroup
