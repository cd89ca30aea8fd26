"""tests/ntt_model.py, the Python-integer transform the NTT tests compare against, proved against the O(n^2) sum that defines it:
every log2n <= 6 on the seven group orders (log2n <= 1 where q - 1 allows no more), with the library's root and with a second
primitive root (its cube), on the domain and on a coset.  The root formula reproduces the smallest non-residues and the
two-adicities the header lists."""
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402
import ntt_model as M  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

TOP = (1 << 256) - 1
# curve -> (two-adicity of q - 1, smallest positive quadratic non-residue)
FACTS = {"bls377": (47, 11), "bls381": (32, 5), "pallas": (32, 5), "vesta": (32, 5), "bn254": (28, 5), "grumpkin": (1, 3), "ed377": (1, 5)}


def sizes(q):
    return range(0, min(6, M.two_adicity(q)) + 1)


def inputs(name, tag, n, q):
    vals = O.prng_ints(f"ntt/model/{name}/{tag}", n, 1 << 256)
    for i, s in zip(range(1, n, 3), (q, q + 1, TOP, 0)):
        vals[i] = s
    return vals


@pytest.mark.parametrize("name", D.NAMES)
def test_root_formula(name):
    q = D.CURVE_TABLE[name].q
    adicity, g = FACTS[name]
    assert M.two_adicity(q) == adicity and M.non_residue(q) == g
    assert M.max_log2n(q) == min(adicity, 29)
    assert all(pow(c, (q - 1) // 2, q) == 1 for c in range(1, g))      # g is the SMALLEST non-residue
    assert M.root_of_unity(q, 0) == 1
    for k in range(1, min(adicity, 29) + 1):
        w = M.root_of_unity(q, k)
        assert w * w % q == M.root_of_unity(q, k - 1)
        assert pow(w, 1 << (k - 1), q) == q - 1                         # order exactly 2^k


@pytest.mark.parametrize("name", D.NAMES)
def test_forward_is_the_defining_sum(name):
    q = D.CURVE_TABLE[name].q
    shift = O.prng_ints(f"ntt/model/{name}/shift", 1, q - 1)[0] + 1
    for log2n in sizes(q):
        n = 1 << log2n
        a = inputs(name, "fwd", n, q)
        lib_root = M.root_of_unity(q, log2n)
        for omega in (lib_root, pow(lib_root, 3, q)):
            if n >= 2:
                assert pow(omega, n // 2, q) == q - 1
            for sh in (1, shift):
                assert M.ntt(a, q, omega, sh) == M.ntt_definition(a, q, omega, sh), (name, log2n, sh != 1)
        assert M.ntt(a, q) == M.ntt_definition(a, q, lib_root)           # omega=None is the library's root


@pytest.mark.parametrize("name", D.NAMES)
def test_inverse_undoes_forward(name):
    q = D.CURVE_TABLE[name].q
    shift = O.prng_ints(f"ntt/model/{name}/shift", 1, q - 1)[0] + 1
    for log2n in sizes(q):
        n = 1 << log2n
        a = inputs(name, "inv", n, q)
        lib_root = M.root_of_unity(q, log2n)
        for omega in (lib_root, pow(lib_root, 3, q)):
            for sh in (1, shift):
                ev = M.ntt(a, q, omega, sh)
                assert M.ntt(ev, q, omega, sh, inverse=True) == [v % q for v in a], (name, log2n)
                assert M.ntt(M.ntt(a, q, omega, sh, inverse=True), q, omega, sh) == [v % q for v in a], (name, log2n)
