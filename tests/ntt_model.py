"""A number-theoretic transform in Python integers: the model msm_scalars_ntt is tested against.

forward:  out[k] = sum_j a[j] (shift omega^k)^j   -- the polynomial with coefficients a on the coset shift <omega>
inverse:  the exact inverse map, the factors n^-1 and shift^-j included
Natural order in and out.  `ntt` is the iterative radix-2 form; `ntt_definition` is the O(n^2) sum it is proved against
(tests/test_ntt_model.py).  Inputs may be any integers: they count as their residues mod q."""


def two_adicity(q: int) -> int:
    s, m = 0, q - 1
    while m % 2 == 0:
        s, m = s + 1, m // 2
    return s


def non_residue(q: int) -> int:
    """the smallest positive quadratic non-residue mod q"""
    g = 2
    while pow(g, (q - 1) // 2, q) != q - 1:
        g += 1
    return g


def root_of_unity(q: int, log2n: int) -> int:
    """the library's primitive 2^log2n-th root: g^((q-1)/2^log2n), g the smallest non-residue"""
    assert log2n <= two_adicity(q)
    return pow(non_residue(q), (q - 1) >> log2n, q)


def max_log2n(q: int) -> int:
    return min(two_adicity(q), 29)


def _bit_reverse(v: int, bits: int) -> int:
    r = 0
    for _ in range(bits):
        r, v = (r << 1) | (v & 1), v >> 1
    return r


def _transform(a, omega: int, q: int):
    n = len(a)
    bits = n.bit_length() - 1
    x = [a[_bit_reverse(i, bits)] % q for i in range(n)]
    half = 1
    while half < n:
        w_step = pow(omega, n // (2 * half), q)
        for start in range(0, n, 2 * half):
            w = 1
            for m in range(half):
                u, t = x[start + m], x[start + m + half] * w % q
                x[start + m], x[start + m + half] = (u + t) % q, (u - t) % q
                w = w * w_step % q
        half *= 2
    return x


def ntt(a, q: int, omega: int = None, shift: int = 1, inverse: bool = False):
    n = len(a)
    assert n and n & (n - 1) == 0
    if omega is None:
        omega = root_of_unity(q, n.bit_length() - 1)
    if n == 1:
        return [a[0] % q]
    if not inverse:
        s, scaled = 1, []
        for v in a:
            scaled.append(v * s % q)
            s = s * shift % q
        return _transform(scaled, omega, q)
    x = _transform(a, pow(omega, q - 2, q), q)
    s, si, out = pow(n, q - 2, q), pow(shift, q - 2, q), []
    for v in x:
        out.append(v * s % q)
        s = s * si % q
    return out


def ntt_definition(a, q: int, omega: int, shift: int = 1):
    """the forward transform as the sum it is defined by, O(n^2)"""
    n = len(a)
    out = []
    for k in range(n):
        x, p, acc = shift * pow(omega, k, q) % q, 1, 0
        for v in a:
            acc = (acc + v * p) % q
            p = p * x % q
        out.append(acc)
    return out
