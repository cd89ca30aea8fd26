#!/usr/bin/env python3
"""Generates tests/golden/cycles_{bn254,grumpkin,vesta}.json: seeded MSM vectors of the two curve cycles from the CPU oracle
(msm_batched_affine, cross-checked here against msm_naive_affine), with the edge cases of SURVEY.md section 8(d).  The files
are kept small (N <= 37 per case): larger sizes are checked on the GPU against the oracle run live and against known discrete logs.
Re-run from the repository root:
    python tests/golden/make_golden_cycles.py
Points are x || y at 32 bytes little-endian each ((0, 0) = the identity), scalars 32 bytes little-endian.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.dirname(HERE)):
    if d not in sys.path:
        sys.path.insert(0, d)
from oracle import msm_oracle as O  # noqa: E402


def case(name, B, scalars, points, c):
    exp = O.msm_batched_affine(scalars, points, B, c=c)
    assert exp == O.msm_naive_affine(scalars, points, B), name
    return {
        "name": name, "c": c,
        "points": O.points_to_bytes([(0, 0) if P is None else P for P in points], 32).hex(),
        "scalars": O.scalars_to_bytes(scalars).hex(),
        "result": None if exp is None else [hex(exp[0]), hex(exp[1])],
    }


def cases(name, B):
    q, p = B.q, B.p
    pts, _ = O.random_points_bls377(f"golden/cycles/{name}", 37, B)
    sc = lambda tag, n: O.prng_ints(f"golden/cycles/{name}/{tag}", n, q)   # noqa: E731
    out = [
        case("n1", B, sc("n1", 1), pts[:1], 4),
        case("zero_scalars", B, [0] * 5, pts[:5], 5),
        case("some_zero_scalars", B, [0, 7, 0, q - 3, 0, 1], pts[:6], 5),
        case("q_minus_1", B, [q - 1, q - 1, 1, q - 2, B.lam, B.lam + 1], pts[:6], 6),
        case("repeated_points", B, sc("rep", 9), [pts[i % 3] for i in range(9)], 4),
        # the same digit in every window for P and -P: both land in the same bucket and cancel there
        case("p_and_minus_p_one_bucket", B, [9, 9, 5], [pts[0], O.aff_neg(pts[0], p), pts[1]], 4),
        case("p_and_minus_p_cancel_to_identity", B, [11, 11], [pts[2], O.aff_neg(pts[2], p)], 3),
        case("all_points_equal", B, sc("eq", 17), [pts[5]] * 17, 5),
        case("all_equal_same_scalar", B, [sc("eq1", 1)[0]] * 8, [pts[6]] * 8, 4),
        case("identity_points", B, sc("inf", 5), [pts[0], None, pts[1], None, pts[2]], 4),
        case("n37", B, sc("n37", 37), pts[:37], 6),     # not a power of two
    ]
    return out


def document(name, B):
    return {"curve": name, "p": hex(B.p), "q": hex(B.q), "b": hex(B.b), "generator": [hex(B.gx), hex(B.gy)], "msm": cases(name, B)}


def main():
    from test_cycle_curves import CURVES

    for name, entry in sorted(CURVES.items()):
        doc = document(name, entry[1])
        path = os.path.join(HERE, f"cycles_{name}.json")
        with open(path, "w") as f:
            json.dump(doc, f, indent=0)
            f.write("\n")
        print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
