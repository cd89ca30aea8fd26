"""The two curve cycles (BN254 G1 / Grumpkin, Pallas / Vesta): what can be checked without a GPU.

* pins that do not depend on the code under test: generators, group orders, the EIP-196 doubling vector, the cycle relations,
  the endomorphism constants;
* montgomery_amd/csrc/constants_gen.h parsed and compared with Python integers and the oracle's GLV parameters;
* the field / square-root / GLV templates of the three curves compiled for the CPU (tests/csrc/field_host_cycles.hip) against
  Python integers;
* the compressed encodings in Python, both ways, with their refusals;
* the committed fixtures tests/golden/cycles_*.json regenerate bit for bit and hold the edge cases.

The constants below are restated from the sources (EIP-196 / the Barretenberg and pasta curve definitions), not imported
from the package, and `oracle/` has no entry for these curves: its generic functions run on WeierstrassParams built here.
"""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from oracle import msm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HDR = os.path.join(ROOT, "montgomery_amd", "csrc", "constants_gen.h")
LIB = os.path.join(ROOT, "tests", "csrc", "libfield_host_cycles.so")

BN254_P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
BN254_Q = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
PALLAS_P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
PALLAS_Q = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001

BN254 = O.WeierstrassParams(
    label="bn254", p=BN254_P, q=BN254_Q, h=1, b=3, gx=1, gy=2,
    lam=0xB3C4D79D41A917585BFC41088D8DAAA78B17EA66B99C90DD, beta=0x59E26BCEA0D48BACD4F263F1ACDB5C4F5763473177FFFFFE, n_bytes=32)
GRUMPKIN = O.WeierstrassParams(
    label="grumpkin", p=BN254_Q, q=BN254_P, h=1, b=BN254_Q - 17, gx=1, gy=0x2CF135E7506A45D632D270D45F1181294833FC48D823F272C,
    lam=0x30644E72E131A0295E6DD9E7E0ACCCB0C28F069FBB966E3DE4BD44E5607CFD48,
    beta=0x30644E72E131A029048B6E193FD84104CC37A73FEC2BC5E9B8CA0B2D36636F23, n_bytes=32)
VESTA = O.WeierstrassParams(
    label="vesta", p=PALLAS_Q, q=PALLAS_P, h=1, b=5, gx=PALLAS_Q - 1, gy=2,
    lam=0x2D33357CB532458ED3552A23A8554E5005270D29D19FC7D27B7FD22F0201B547,
    beta=0x397E65A7D7C1AD71AEE24B27E308F0A61259527EC1D4752E619D1840AF55F1B1, n_bytes=32)

# name -> (curve id of include/msm_hip.h, parameters, field struct, GLV struct, MAX_BITS, 2-adicity of p - 1, pasta encoding?)
CURVES = {
    "bn254": (4, BN254, "FpBn254", "GlvBn254", 126, 1, False),
    "grumpkin": (5, GRUMPKIN, "FpGrumpkin", "GlvGrumpkin", 126, 28, False),
    "vesta": (6, VESTA, "FpVesta", "GlvVesta", 127, 32, True),
}
NAMES = sorted(CURVES)
NL, NW = 9, 8
R = 1 << (30 * NL)


# ---------------------------------------------------------------------------------------------- pins

@pytest.mark.parametrize("name", NAMES)
def test_generator_order_and_endomorphism(name):
    B = CURVES[name][1]
    G = (B.gx, B.gy)
    assert (B.gy * B.gy - B.gx ** 3 - B.b) % B.p == 0
    assert O.aff_is_on_curve(G, B)
    assert O.aff_scale(B.q, G, B.p) is None and O.aff_scale(B.q - 1, G, B.p) == O.aff_neg(G, B.p)
    assert B.lam != 1 and pow(B.lam, 3, B.q) == 1 and B.beta != 1 and pow(B.beta, 3, B.p) == 1
    assert O.aff_scale(B.lam, G, B.p) == (B.beta * B.gx % B.p, B.gy)


def test_bn254_doubling_is_the_eip196_vector():
    assert O.aff_scale(2, (1, 2), BN254_P) == (0x030644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD3,
                                               0x15ED738C0E0A7C92E7845F96B2AE9C0A68A6A449E3538FC7FF3EBF7A5A18A2C4)


def test_cycle_relations():
    assert (GRUMPKIN.p, GRUMPKIN.q) == (BN254.q, BN254.p)
    assert (VESTA.p, VESTA.q) == (O.PALLAS.q, O.PALLAS.p) == (PALLAS_Q, PALLAS_P)
    assert BN254.p.bit_length() == BN254.q.bit_length() == 254 and VESTA.p.bit_length() == 255
    assert BN254.p % 4 == 3 and BN254.p % (1 << 30) != 1 and GRUMPKIN.p % (1 << 30) != 1 and VESTA.p % (1 << 30) == 1
    assert GRUMPKIN.b == GRUMPKIN.p - 17


# ---------------------------------------------------------------------------------------------- constants_gen.h

def parse_struct(name):
    with open(HDR) as f:
        text = f.read()
    m = re.search(r"struct %s \{(.*?)\n\};" % name, text, re.S)
    assert m, f"constants_gen.h has no struct {name}"
    body = m.group(1)
    out = {}
    for k, v in re.findall(r"static constexpr (?:int|uint32_t) (\w+) = (0x[0-9a-f]+|\d+)u?;", body):
        out[k] = int(v, 0)
    for k, n, vals in re.findall(r"static constexpr uint32_t (\w+)\[(\d+)\] = \{([^}]*)\};", body):
        out[k] = [int(x.strip().rstrip("u"), 16) for x in vals.split(",")]
        assert len(out[k]) == int(n)
    return out


def join(vals, bits):
    assert all(0 <= v < (1 << bits) for v in vals)
    return sum(v << (bits * i) for i, v in enumerate(vals))


@pytest.mark.parametrize("name", NAMES)
def test_generated_field_constants(name):
    _, B, fs, _, _, two_adicity, _ = CURVES[name]
    S = parse_struct(fs)
    p = B.p
    assert (S["NL"], S["NW"], S["NLA"], S["BITS"]) == (NL, NW, NL, p.bit_length())
    assert R > 64 * p                                   # every value the kernels form fits the active limbs
    assert join(S["P"], 30) == p == join(S["PW"], 32)
    assert join(S["P2"], 30) == 2 * p and join(S["P4"], 30) == 4 * p
    assert S["MU"] == (-pow(p, -1, 1 << 30)) % (1 << 30) and S["PINV30"] == pow(p, -1, 1 << 30)
    assert join(S["ONE"], 30) == R % p == join(S["ONEW"], 32)
    assert join(S["R2"], 30) == R * R % p == join(S["R2W"], 32)
    assert join(S["R3"], 30) == R ** 3 % p
    assert join(S["PM2W"], 32) == p - 2 and join(S["HALFW"], 32) == (p - 1) // 2
    assert join(S["BL"], 30) == B.b * R % p == join(S["BW"], 32)
    assert join(S["BETAL"], 30) == B.beta * R % p and join(S["GXW"], 32) == B.gx * R % p and join(S["GYW"], 32) == B.gy * R % p
    assert S["TWO_ADICITY"] == two_adicity and (p - 1) % (1 << two_adicity) == 0 and ((p - 1) >> two_adicity) & 1
    t = (p - 1) >> two_adicity
    e = join(S["SQRT_EW"], 32)
    assert e == ((p + 1) // 4 if two_adicity == 1 else (t - 1) // 2) and S["SQRT_EBITS"] == e.bit_length()
    if two_adicity > 1:   # z = g^t R: a primitive 2^S-th root of unity
        z = join(S["SQRT_ZL"], 30) * pow(R, -1, p) % p
        assert pow(z, 1 << (two_adicity - 1), p) == p - 1


@pytest.mark.parametrize("name", NAMES)
def test_generated_glv_constants(name):
    _, B, _, gs, max_bits, _, _ = CURVES[name]
    S = parse_struct(gs)
    g = O.glv_params(B.q, B.lam)
    assert g.max_bits == max_bits == S["MAX_BITS"]
    assert (S["M_SHIFT"], S["K_SHIFT"]) == (g.m, g.k)
    for key, v in (("V00", g.v00), ("V01", g.v01), ("V10", g.v10), ("V11", g.v11), ("M0", g.m0), ("M1", g.m1)):
        assert join(S[key], 32) == abs(v) and S[key + "_NEG"] == (1 if v < 0 else 0), key
    assert join(S["Q"], 32) == B.q
    # the lattice: both rows are multiples of (lambda, -1) mod q, i.e. v_0 + lambda v_1 = 0
    assert (g.v00 + B.lam * g.v10) % B.q == 0 and (g.v01 + B.lam * g.v11) % B.q == 0


def test_accumulators_need_no_guard_sweep():
    """A Python copy of fe_acc_fits (field.h) at guard_row = -1: the 64-bit column accumulators of the interleaved product
    and square hold the worst case (all limbs and quotient digits 2^30 - 1) for the three fields."""
    M, LIM = (1 << 30) - 1, 1 << 64
    for name in NAMES:
        P = parse_struct(CURVES[name][2])["P"]
        for sqr in (False, True):
            w = [0] * NL
            for i in range(NL):
                for j in range(i if sqr else 0, NL):
                    w[j] += M * 2 * M if (sqr and j > i) else M * M
                assert max(w) < LIM and w[0] + M * P[0] < LIM
                carry = ((w[0] + M * P[0]) >> 30) + 1
                for j in range(1, NL):
                    w[j] += M * P[j]
                w[1] += carry
                assert max(w) < LIM, (name, sqr, i)
                w = w[1:] + [0]


# ---------------------------------------------------------------------------------------------- host build of the templates

@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", ROOT, "-s", "hosttest"])   # own shim library, never loaded by anything else
    lib = C.CDLL(LIB)
    for fn in (lib.cyc_fp_op, lib.cyc_fp_raw):
        fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cyc_glv.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.cyc_packed.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def fp_op(lib, cid, which, a, b=0):
    A = (C.c_uint32 * NW)(*[(a >> (32 * i)) & 0xFFFFFFFF for i in range(NW)])
    Bv = (C.c_uint32 * NW)(*[(b >> (32 * i)) & 0xFFFFFFFF for i in range(NW)])
    out = (C.c_uint32 * NW)()
    flag = lib.cyc_fp_op(cid, which, A, Bv, out)
    assert flag >= 0
    return flag, sum(int(w) << (32 * i) for i, w in enumerate(out))


def field_values(name, p, count):
    """Canonical values, and values in [p, 2p): the operand contract of every operation of the shim allows them."""
    return [0, 1, 2, 3, p - 1, p - 2, (p + 1) // 2, (1 << 30) - 1, 1 << 30, 1 << 253, p, p + 1, 2 * p - 1, p + (1 << 200)] + \
        O.prng_ints(f"cycles/host/{name}", count, p)


@pytest.mark.parametrize("name", NAMES)
def test_host_mul_sqr_add_sub(lib, name):
    cid, B = CURVES[name][:2]
    p, rinv = B.p, pow(R, -1, B.p)
    vals = field_values(name, p, 300)
    for i, a in enumerate(vals):
        b = vals[-1 - i]
        assert fp_op(lib, cid, 0, a, b)[1] == a * b * rinv % p
        assert fp_op(lib, cid, 1, a)[1] == a * a * rinv % p
        assert fp_op(lib, cid, 2, a, b)[1] == (a + b) % p       # packed in, fe_add, reduced and packed out
        assert fp_op(lib, cid, 3, a, b)[1] == (a - b) % p       # fe_sub_2p: b < 2p
        assert fp_op(lib, cid, 9, a)[1] == a * rinv % p         # fe_plain_words: out of Montgomery form, canonical


def packed_edge_values(p):
    """Packed-word operands at the edges: 0, 1, p - 1, values whose difference borrows or carries across every 32-bit word
    boundary, and the top of the canonical range."""
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    for k in range(1, NW):
        vals += [(1 << (32 * k)) - 1, 1 << (32 * k), (1 << (32 * k)) + 1]
    vals += [p - (1 << 32), p - (1 << 224), (1 << 253) - 1, 1 << 253]
    return sorted({v for v in vals if 0 <= v < p})


@pytest.mark.parametrize("name", NAMES)
def test_host_packed_add_sub(lib, name):
    """pk_sub_mod, pk_cond_sub_p, pk_add and pk_sub of packed.h (the plain C++ chains of a CPU build) on a 254- / 255-bit modulus
    in 8 words: a in [0, p + eps) and beyond (anything below 2^256 the contracts allow), b in [0, p)."""
    cid, B = CURVES[name][:2]
    p, M = B.p, 1 << 256

    def pk(which, a, b=0):
        A = (C.c_uint32 * NW)(*[(a >> (32 * i)) & 0xFFFFFFFF for i in range(NW)])
        Bv = (C.c_uint32 * NW)(*[(b >> (32 * i)) & 0xFFFFFFFF for i in range(NW)])
        out, borrow = (C.c_uint32 * NW)(), C.c_uint32()
        assert lib.cyc_packed(cid, which, A, Bv, out, C.byref(borrow)) == 0
        return sum(int(w) << (32 * i) for i, w in enumerate(out)), borrow.value

    edge = packed_edge_values(p)
    rnd = O.prng_ints(f"cycles/packed/{name}", 40, p)
    for a in edge + rnd:
        for b in edge + rnd[:6]:
            assert pk(0, a, b)[0] == (a - b) % p, (hex(a), hex(b))            # canonical operands: canonical result
            assert pk(3, a, b) == ((a - b) % M, 0xFFFFFFFF if a < b else 0)   # the raw chain and its borrow mask
            assert pk(2, a, b)[0] == (a + b) % M
        for eps in (0, 1, 5, 1 << 32, p - 1):                                 # a in [p, 2p): pk_sub_mod keeps the excess
            a2 = a + eps if eps < p - 1 else a + p
            if a2 < M:
                for b in edge[:8] + edge[-4:]:
                    r = pk(0, a2, b)[0]
                    assert r % p == (a2 - b) % p and r <= max(a2, p - 1), (hex(a2), hex(b))   # a2 - b, or a2 - b + p < p
        for r in (a, a + p):                                                  # pk_cond_sub_p: r < 2p -> r mod p
            if r < M:
                assert pk(1, r)[0] == r % p
    assert pk(1, p)[0] == 0 and pk(1, p - 1)[0] == p - 1 and pk(1, 2 * p - 1)[0] == p - 1


@pytest.mark.parametrize("name", NAMES)
def test_host_four_inversions(lib, name):
    """fe_inv (division steps, p^-1 != 1 mod 2^30 at 9 limbs for BN254 / Grumpkin) == Fermat == Kaliski == word-sliced."""
    cid, B = CURVES[name][:2]
    p = B.p
    vals = field_values(name, p, 300) + [1 << 200, (1 << 252) - 1, (1 << 117) - 1, (1 << 253) + 1]
    for k, a in enumerate(vals):
        if a % p == 0:   # 0 gives 0; p itself, the other representative of zero below 2p, is not an input of any kernel
            assert a != 0 or fp_op(lib, cid, 4, a)[1] == 0
            continue
        exp = pow(a, -1, p) * R * R % p
        assert fp_op(lib, cid, 4, a)[1] == exp, hex(a)
        if k < 120:
            assert fp_op(lib, cid, 6, a)[1] == exp and fp_op(lib, cid, 7, a)[1] == exp, hex(a)
        if k < 40:
            assert fp_op(lib, cid, 5, a)[1] == exp, hex(a)
    assert fp_op(lib, cid, 6, 0)[1] == 0 and fp_op(lib, cid, 7, 0)[1] == 0


@pytest.mark.parametrize("name", NAMES)
def test_host_square_root(lib, name):
    """fe_sqrt: p = 3 mod 4 (BN254), Tonelli-Shanks with 2-adicity 28 (Grumpkin) and 32 (Vesta); squares, non-squares, 0,
    and elements of high 2-power order (powers of the 2^S-th root of unity), which walk every level of the loop."""
    cid, B = CURVES[name][:2]
    p, rinv = B.p, pow(R, -1, B.p)
    S = CURVES[name][5]
    g = next(x for x in range(2, 50) if pow(x, (p - 1) // 2, p) == p - 1)
    z = pow(g, (p - 1) >> S, p)
    vals = field_values(name, p, 200) + [pow(z, 1 << k, p) for k in range(S)] + [v * v % p for v in O.prng_ints(f"cycles/sq/{name}", 50, p)]
    n_sq = 0
    for x in vals:
        a = x * R % p if x < p else x       # Montgomery form of x (values >= p go in as they are: any value < 2p)
        plain = a * rinv % p
        ok, r = fp_op(lib, cid, 8, a)
        assert bool(ok) == (plain == 0 or pow(plain, (p - 1) // 2, p) == 1), hex(x)
        if ok:
            n_sq += 1
            root = r * rinv % p
            assert r < p and root * root % p == plain
    assert 50 < n_sq < len(vals)


def limb_operands(p, seed):
    """Operands the kernels feed the multiplier (a b < 2^12 p^2, limbs normalised): sums of a few elements up to 64 p, values
    next to multiples of p, and limb patterns that maximise the column sums."""
    vals = [0, 1, p - 1, p, p + 1, 2 * p - 1, 4 * p - 3, 63 * p, 64 * p - 1, (1 << (30 * (NL - 1))) - 1]
    vals.append((1 << ((64 * p).bit_length() - 1)) - 1)
    vals += [v * k + d for v in O.prng_ints(f"cycles/raw/{seed}", 60, p) for k, d in ((1, 0), (7, 3), (63, 0))]
    return [v for v in vals if v < 64 * p]


@pytest.mark.parametrize("name", NAMES)
def test_host_raw_multiplier_on_unreduced_and_all_ones_limbs(lib, name):
    cid, B = CURVES[name][:2]
    p, rinv = B.p, pow(R, -1, B.p)

    def raw(which, a, b):
        A = (C.c_uint32 * NL)(*[(a >> (30 * i)) & 0x3FFFFFFF if i < NL - 1 else a >> (30 * i) for i in range(NL)])
        Bv = (C.c_uint32 * NL)(*[(b >> (30 * i)) & 0x3FFFFFFF if i < NL - 1 else b >> (30 * i) for i in range(NL)])
        out = (C.c_uint32 * NL)()
        assert lib.cyc_fp_raw(cid, which, A, Bv, out) == 0
        assert all(int(w) < (1 << 30) for w in out[: NL - 1]), "limbs not normalised"
        return sum(int(w) << (30 * i) for i, w in enumerate(out))

    vals = limb_operands(p, name)
    for i, a in enumerate(vals):
        b = vals[-1 - i]
        r = raw(0, a, b)
        assert r % p == a * b * rinv % p and r < p + a * b // R + 1
        r = raw(1, a, a)
        assert r % p == a * a * rinv % p and r < p + a * a // R + 1
    ones = R - 1   # beyond the contract: no accumulator may wrap, the value is still congruent
    assert raw(0, ones, ones) % p == ones * ones * rinv % p
    assert raw(1, ones, ones) % p == ones * ones * rinv % p


@pytest.mark.parametrize("name", NAMES)
def test_host_glv_decompose(lib, name):
    cid, B = CURVES[name][:2]
    g = O.glv_params(B.q, B.lam)
    worst = 0
    for s in O.prng_ints(f"cycles/glv/{name}", 3000, B.q) + [0, 1, 2, B.q - 1, B.q - 2, B.lam, B.lam - 1, B.lam + 1, B.q // 2, 1 << 253]:
        Sv = (C.c_uint32 * 8)(*[(s >> (32 * i)) & 0xFFFFFFFF for i in range(8)])
        out = (C.c_uint32 * 10)()
        assert lib.cyc_glv(cid, Sv, out) == 0
        a0 = sum(int(out[i]) << (32 * i) for i in range(4))
        a1 = sum(int(out[4 + i]) << (32 * i) for i in range(4))
        assert (a0, a1, bool(out[8]), bool(out[9])) == O.glv_decompose(s, g), hex(s)
        assert ((-a0 if out[8] else a0) + B.lam * (-a1 if out[9] else a1) - s) % B.q == 0
        worst = max(worst, a0.bit_length(), a1.bit_length())
    assert worst <= g.max_bits


# ---------------------------------------------------------------------------------------------- compressed encodings

def compress(name, P):
    """The encodings of include/msm_hip.h (msm_set_points_ex): arkworks at 32 bytes for BN254 / Grumpkin, pasta for Vesta."""
    B, pasta = CURVES[name][1], CURVES[name][6]
    if P is None:
        return bytes(32) if pasta else bytes(31) + b"\x40"
    x, y = P
    sign = (y & 1) if pasta else int(y > (B.p - 1) // 2)
    return (x | (sign << 255)).to_bytes(32, "little")


def decompress(name, buf, B=None):
    """-> point, None (identity), or the refusal reason as the library words it.  B: other parameters under the same rules."""
    B, pasta = B or CURVES[name][1], CURVES[name][6]
    v = int.from_bytes(buf, "little")
    sign = v >> 255
    if pasta:
        x = v & ((1 << 255) - 1)
        if x == 0 and not sign:
            return None
    else:
        inf, x = (v >> 254) & 1, v & ((1 << 254) - 1)
        if inf:
            return "invalid flags" if (sign or x) else None
    if x >= B.p:
        return "coordinate >= p"
    y = O.sqrt_mod((x ** 3 + B.b) % B.p, B.p)
    if y is None:
        return "no curve point"
    if ((y & 1) if pasta else int(y > (B.p - 1) // 2)) != sign:
        if y == 0:
            return "invalid flags"
        y = B.p - y
    return (x, y)


@pytest.mark.parametrize("name", NAMES)
def test_codec_round_trips_and_refusals(name):
    B, pasta = CURVES[name][1], CURVES[name][6]
    pts, _ = O.random_points_bls377(f"cycles/codec/{name}", 40, B)
    pts += [O.aff_neg(P, B.p) for P in pts[:8]] + [(B.gx, B.gy), None]
    for P in pts:
        enc = compress(name, P)
        assert len(enc) == 32 and decompress(name, enc) == P
        if P is not None:   # the other sign bit is the negated point
            flipped = bytes(enc[:31]) + bytes([enc[31] ^ 0x80])
            assert decompress(name, flipped) == O.aff_neg(P, B.p)
    # x >= p
    assert decompress(name, B.p.to_bytes(32, "little")) == "coordinate >= p"
    assert decompress(name, (B.p + 5).to_bytes(32, "little")) == "coordinate >= p"
    # an x without a point
    x = next(x for x in range(2, 200) if O.sqrt_mod((x ** 3 + B.b) % B.p, B.p) is None)
    assert decompress(name, x.to_bytes(32, "little")) == "no curve point"
    if pasta:
        assert decompress(name, bytes(32)) is None
        assert decompress(name, bytes(31) + b"\x80") == "no curve point"      # x = 0 with the sign bit: 5 is no square
        assert O.sqrt_mod(5, B.p) is None
    else:
        assert decompress(name, bytes(31) + b"\x40") is None
        assert decompress(name, bytes(31) + b"\xc0") == "invalid flags"          # both flags
        assert decompress(name, b"\x01" + bytes(30) + b"\x40") == "invalid flags"  # infinity with x bits
    # the sign bit on a zero root.  y = 0 is a point of order 2, which a group of odd prime order does not have, so no input
    # reaches that rule on these curves; it is exercised under the same encoding on y^2 = x^3 - 1, where x = 1 has the root 0
    assert B.q % 2 == 1
    import dataclasses

    toy = dataclasses.replace(B, b=B.p - 1)
    assert decompress(name, (1).to_bytes(32, "little"), toy) == (1, 0)
    assert decompress(name, (1 | (1 << 255)).to_bytes(32, "little"), toy) == "invalid flags"


# ---------------------------------------------------------------------------------------------- fixtures

@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_reproducible_and_has_the_edge_cases(name):
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_golden_cycles", os.path.join(GOLD, "make_golden_cycles.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLD, f"cycles_{name}.json")) as f:
        gold = json.load(f)
    B = CURVES[name][1]
    assert gold == json.loads(json.dumps(mod.document(name, B)))     # seeded: regenerates bit for bit (and cross-checks there)
    names = {c["name"] for c in gold["msm"]}
    assert {"zero_scalars", "q_minus_1", "repeated_points", "p_and_minus_p_one_bucket", "all_points_equal", "n1", "n37"} <= names
    for c in gold["msm"]:   # independent of the generator: the plain double-and-add sum of what the file holds
        n = len(c["scalars"]) // 64
        assert n <= 1 << 10 and len(c["points"]) == 128 * n
        sc = O.scalars_from_bytes(bytes.fromhex(c["scalars"]))
        pts = [None if P == (0, 0) else P for P in O.points_from_bytes(bytes.fromhex(c["points"]), 32)]
        exp = O.msm_naive_affine(sc, pts, B)
        assert (None if c["result"] is None else (int(c["result"][0], 16), int(c["result"][1], 16))) == exp, c["name"]
