"""Host-side mirror of the reference's curve-module API for the MSM path.

Reference surface being mirrored (names, argument meaning, error behaviour):
  * ``Weierstraß.create(params)``                      src/parallel.ts:40-177
  * ``Curve.Parallel.{msm, msmUnsafe, pointsFromBytes, scalarsFromBytes, getPointer,
    getScalarPointer, randomPointsFast, randomScalars}``   src/parallel.ts:135-145
  * ``msm(scalarPtr, pointPtr, N, verbose, {c, useSafeAdditions}) -> {result, log}``
                                                        src/msm-batched-affine.ts:69-78, :339
  * ``compute_msm(points, scalars) -> {x, y}``          scripts/zprize23/submission-bls377.ts:20-65

In the reference "pointers" are byte offsets into the shared wasm memory; here they are small handle
objects for buffers owned by the HIP library (points live in HBM in the library's row format, scalars
either on the host or in HBM).  All arithmetic happens in libmsm_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

from . import _lib
from ._lib import MsmError, MsmOpts, MsmResult

BytesLike = Union[bytes, bytearray, memoryview]


# ---------------------------------------------------------------------------------------------
# curve parameters (src/concrete/bls12-377.params.ts:11-45)
# ---------------------------------------------------------------------------------------------


@dataclass(frozen=True)
class WeierstrassParams:
    label: str
    modulus: int
    order: int
    cofactor: int
    a: int
    b: int
    generator: Tuple[int, int]
    endomorphism: Tuple[int, int]  # (lambda, beta)


BLS12_377_PARAMS = WeierstrassParams(
    label="bls12-377",
    modulus=0x01AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001,
    order=0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001,
    cofactor=0x170B5D44300000000000000000000000,
    a=0,
    b=1,
    generator=(
        0x008848DEFE740A67C8FC6225BF87FF5485951E2CAA9D41BB188282C8BD37CB5CD5481512FFCD394EEAB9B16EB21BE9EF,
        0x01914A69C5102EFF1F674F5D30AFEEC4BD7FB348CA3E52D96D182AD44FB82305C2FE3D3634A9591AFD82DE55559C8EA6,
    ),
    endomorphism=(
        0x12AB655E9A2CA55660B44D1E5C37B00114885F32400000000000000000000000,
        0x1AE3A4617C510EABC8756BA8F8C524EB8882A75CC9BC8E359064EE822FB5BFFD1E945779FFFFFFFFFFFFFFFFFFFFFFF,
    ),
)


BLS12_381_PARAMS = WeierstrassParams(  # src/concrete/bls12-381.params.ts:6-55
    label="bls12-381",
    modulus=0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
    order=0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
    cofactor=0x396C8C005555E1568C00AAAB0000AAAB,
    a=0,
    b=4,
    generator=(
        0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
        0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1,
    ),
    endomorphism=(
        0xD201000000010000 ** 2 - 1,
        0x1A0111EA397FE699EC02408663D4DE85AA0D857D89759AD4897D29650FB85F9B409427EB4F49FFFD8BFD00000000AAAC,
    ),
)

_PALLAS_P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
_PALLAS_Q = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
PALLAS_PARAMS = WeierstrassParams(  # src/concrete/pasta.params.ts:10-53
    label="pallas",
    modulus=_PALLAS_P,
    order=_PALLAS_Q,
    cofactor=1,
    a=0,
    b=5,
    generator=(1, 0x1B74B5A30A12937C53DFA9F06378EE548F655BD4333D477119CF7A23CAED2ABB),
    endomorphism=(pow(5, (_PALLAS_Q - 1) // 3, _PALLAS_Q), pow(pow(5, (_PALLAS_P - 1) // 3, _PALLAS_P), 2, _PALLAS_P)),
)

# The two curve cycles of recursive provers (not in the reference).  BN254 G1 is alt_bn128 of EIP-196; Grumpkin swaps its two
# fields, Vesta swaps those of Pallas.  (lambda, beta): the cube roots of unity with lambda G = (beta x, y).
_BN254_P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
_BN254_Q = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
BN254_PARAMS = WeierstrassParams(
    label="bn254",
    modulus=_BN254_P,
    order=_BN254_Q,
    cofactor=1,
    a=0,
    b=3,
    generator=(1, 2),
    endomorphism=(0xB3C4D79D41A917585BFC41088D8DAAA78B17EA66B99C90DD, 0x59E26BCEA0D48BACD4F263F1ACDB5C4F5763473177FFFFFE),
)
GRUMPKIN_PARAMS = WeierstrassParams(
    label="grumpkin",
    modulus=_BN254_Q,
    order=_BN254_P,
    cofactor=1,
    a=0,
    b=_BN254_Q - 17,
    generator=(1, 0x2CF135E7506A45D632D270D45F1181294833FC48D823F272C),
    endomorphism=(0x30644E72E131A0295E6DD9E7E0ACCCB0C28F069FBB966E3DE4BD44E5607CFD48,
                  0x30644E72E131A029048B6E193FD84104CC37A73FEC2BC5E9B8CA0B2D36636F23),
)
VESTA_PARAMS = WeierstrassParams(
    label="vesta",
    modulus=_PALLAS_Q,
    order=_PALLAS_P,
    cofactor=1,
    a=0,
    b=5,
    generator=(_PALLAS_Q - 1, 2),
    endomorphism=(0x2D33357CB532458ED3552A23A8554E5005270D29D19FC7D27B7FD22F0201B547,
                  0x397E65A7D7C1AD71AEE24B27E308F0A61259527EC1D4752E619D1840AF55F1B1),
)
BN254, GRUMPKIN, VESTA = BN254_PARAMS, GRUMPKIN_PARAMS, VESTA_PARAMS   # Weierstrass.create(BN254), compute_msm(..., BN254)

# curves with device constants (montgomery_amd/csrc/constants_gen.h), by label
_WEIERSTRASS_CURVE_IDS = {"bls12-377": _lib.CURVE_BLS12_377_G1, "bls12-381": _lib.CURVE_BLS12_381_G1,
                          "pallas": _lib.CURVE_PALLAS, "bn254": _lib.CURVE_BN254_G1, "grumpkin": _lib.CURVE_GRUMPKIN,
                          "vesta": _lib.CURVE_VESTA}


@dataclass(frozen=True)
class TwistedEdwardsParams:
    """src/concrete/ed-on-bls12-377.params.ts:5-31"""

    label: str
    modulus: int
    order: int
    cofactor: int
    d: int
    generator: Tuple[int, int]


ED_ON_BLS12_377_PARAMS = TwistedEdwardsParams(
    label="ed-on-bls12-377",
    modulus=0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001,
    order=0x4AAD957A68B2955982D1347970DEC005293A3AFC43C8AFEB95AEE9AC33FD9FF,
    cofactor=4,
    d=3021,
    generator=(
        0x9F1B5A5BAF6ACF06FED91C9AE9EBFA06068DD2835790980894E2328F3EBCA05,
        0x9A20DF36571AC3CD906B256080BA8454453C177AAF3131BB50A67BF1A806781,
    ),
)



# ---------------------------------------------------------------------------------------------
# indexed (sparse) MSM: host-side input handling (msm_run_indexed, include/msm_hip.h)
# ---------------------------------------------------------------------------------------------


def _as_numpy(a):
    """numpy view of a numpy array or a torch tensor (copied to the host); anything else is returned as it is."""
    if hasattr(a, "detach") and hasattr(a, "cpu"):   # torch.Tensor, without importing torch
        return a.detach().cpu().numpy()
    return a


def _index_array(indices, m: Optional[int] = None):
    """Indices of an indexed call as a contiguous little-endian uint32 array: a 1-d integer numpy array / torch tensor or a
    sequence of ints, none negative, all below 2^32; m: the length the scalars ask for.  (Whether they are below the resident
    count is checked on the GPU, which names the first bad position.)"""
    import numpy as np

    a = _as_numpy(indices)
    if not hasattr(a, "dtype"):
        vals = list(a)
        if any(not isinstance(v, (int, np.integer)) or isinstance(v, bool) for v in vals):
            raise MsmError(_lib.MSM_ERR_ARG, "indices must be integers")
        if any(v < 0 or v >> 32 for v in vals):
            raise MsmError(_lib.MSM_ERR_ARG, "indices must lie in [0, 2^32)")
        a = np.array(vals, dtype="<u4")
    if a.dtype.kind not in "iu":
        raise MsmError(_lib.MSM_ERR_ARG, f"indices must have an integer dtype, got {a.dtype}")
    if a.ndim != 1:
        raise MsmError(_lib.MSM_ERR_ARG, f"indices must be one-dimensional, got shape {a.shape}")
    if a.size and (int(a.min()) < 0 or int(a.max()) >> 32):
        raise MsmError(_lib.MSM_ERR_ARG, "indices must lie in [0, 2^32)")
    if m is not None and a.size != m:
        raise MsmError(_lib.MSM_ERR_ARG, f"{m} scalars but {a.size} indices")
    if a.size >> 30:
        raise MsmError(_lib.MSM_ERR_ARG, "an indexed call takes fewer than 2^30 entries")
    return np.ascontiguousarray(a, dtype="<u4")


def _wide_scalar_bytes(scalars) -> bytes:
    """32-byte scalars of an indexed call: bytes of m x 32, or a uint8 array / tensor of shape (m, 32) or (32 m,)."""
    a = _as_numpy(scalars)
    if hasattr(a, "dtype"):
        import numpy as np

        if a.dtype != np.uint8 or a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] != 32):
            raise MsmError(_lib.MSM_ERR_ARG, f"32-byte scalars must be bytes or a uint8 array of shape (m, 32), got {a.dtype} {a.shape}")
        raw = np.ascontiguousarray(a).tobytes()
    else:
        raw = bytes(a)
    if len(raw) % 32:
        raise MsmError(_lib.MSM_ERR_ARG, f"scalar buffer length {len(raw)} is not a multiple of 32")
    return raw


def sparse_from_dense(scalars):
    """(indices, nonzero_scalars) of a dense scalar vector: the positions of its non-zero scalars as a uint32 array, ascending,
    and those scalars in the same order -- what msm_indexed takes in place of the vector.  scalars: bytes of n x 32 (or a
    uint8 array of shape (n, 32)) -> bytes of m x 32; an integer numpy array (narrow scalars) -> the array of its non-zeros."""
    import numpy as np

    a = _as_numpy(scalars)
    if hasattr(a, "dtype") and not (a.dtype == np.uint8 and a.ndim == 2):
        if a.dtype.kind not in "iu" or a.ndim != 1:
            raise MsmError(_lib.MSM_ERR_ARG, f"a dense vector is bytes, a uint8 array (n, 32) or a 1-d integer array, got {a.dtype} {a.shape}")
        idx = np.flatnonzero(a)
        if idx.size >> 32:
            raise MsmError(_lib.MSM_ERR_ARG, "more than 2^32 - 1 positions")
        return idx.astype("<u4"), np.ascontiguousarray(a[idx])
    rows = np.frombuffer(_wide_scalar_bytes(a), dtype=np.uint8).reshape(-1, 32)
    idx = np.flatnonzero(rows.any(axis=1))
    return idx.astype("<u4"), rows[idx].tobytes()


def dense_from_sparse(indices, scalars: BytesLike, n: int, q: int) -> bytes:
    """The dense equivalent of an indexed call over n points: t[i] = sum of scalars[j] over indices[j] == i, mod q, as n x 32
    bytes -- the vector msm_run gives the same result for (tests, tools/bench_indexed.py)."""
    idx = _index_array(indices)
    raw = _wide_scalar_bytes(scalars)
    if len(raw) != 32 * idx.size:
        raise MsmError(_lib.MSM_ERR_ARG, f"{len(raw) // 32} scalars but {idx.size} indices")
    t = [0] * n
    for j, i in enumerate(idx.tolist()):
        if i >= n:
            raise MsmError(_lib.MSM_ERR_ARG, f"indices[{j}] = {i} but {n} points")
        t[i] = (t[i] + int.from_bytes(raw[32 * j:32 * j + 32], "little")) % q
    return b"".join(v.to_bytes(32, "little") for v in t)

def _scalar32(v, what: str = "scalar") -> bytes:
    """One scalar of msm_points_lincomb as 32 little-endian bytes: an int in [0, 2^256) or 32 bytes.  (Whether it is below q is
    the library's check: MSM_ERR_SCALAR.)"""
    if isinstance(v, bool):
        raise MsmError(_lib.MSM_ERR_ARG, f"{what} must be an int or 32 bytes")
    if isinstance(v, int):
        if v < 0 or v >> 256:
            raise MsmError(_lib.MSM_ERR_ARG, f"{what} must lie in [0, 2^256)")
        return v.to_bytes(32, "little")
    try:
        raw = bytes(v)
    except TypeError:
        raise MsmError(_lib.MSM_ERR_ARG, f"{what} must be an int or 32 bytes") from None
    if len(raw) != 32:
        raise MsmError(_lib.MSM_ERR_ARG, f"{what} must be 32 bytes, got {len(raw)}")
    return raw


@dataclass
class CsrMatrix:
    """A sparse matrix in CSR on the host, as msm_matrix_create takes it: row_ptr (rows + 1 entries), col (nnz column indices) and
    val (nnz x 32 bytes little-endian, or None: every coefficient is 1)."""
    rows: int
    cols: int
    row_ptr: List[int]
    col: List[int]
    val: Optional[bytes]

    @property
    def nnz(self) -> int:
        return len(self.col)


def matrix_from_triplets(rows: int, cols: int, triplets, transpose: bool = False) -> CsrMatrix:
    """(row, col, value) triples -> CSR, by a stable sort over the rows: within a row the entries keep the order of the triples,
    and duplicates are kept (the product sums them).  value: an int in [0, 2^256) or 32 bytes; triples (row, col) without a value,
    or with None in every one, give the all-ones form.  transpose: the CSR of the transposed matrix, cols x rows."""
    trip = [tuple(t) for t in triplets]
    ones = all(len(t) == 2 or t[2] is None for t in trip)
    if not ones and any(len(t) != 3 or t[2] is None for t in trip):
        raise MsmError(_lib.MSM_ERR_ARG, "matrix_from_triplets: every triple carries a value, or none does")
    if transpose:
        trip = [(t[1], t[0]) + t[2:] for t in trip]
        rows, cols = cols, rows
    for j, t in enumerate(trip):
        if not (0 <= t[0] < rows and 0 <= t[1] < cols):
            raise MsmError(_lib.MSM_ERR_ARG, f"matrix_from_triplets: triple {j} lies outside the {rows} x {cols} matrix")
    order = sorted(range(len(trip)), key=lambda j: trip[j][0])   # stable
    row_ptr = [0] * (rows + 1)
    for t in trip:
        row_ptr[t[0] + 1] += 1
    for r in range(rows):
        row_ptr[r + 1] += row_ptr[r]
    col = [trip[j][1] for j in order]
    val = None if ones else b"".join(_scalar32(trip[j][2], "a value") for j in order)
    return CsrMatrix(rows, cols, row_ptr, col, val)


# ---------------------------------------------------------------------------------------------
# low-level context
# ---------------------------------------------------------------------------------------------


@dataclass
class AffineResult:
    """Canonical affine result, as `Affine.toBigint` returns it (src/curve-affine.ts:220-233)."""

    x: int
    y: int
    isZero: bool

    def as_tuple(self) -> Optional[Tuple[int, int]]:
        return None if self.isZero else (self.x, self.y)


def _result_to_dict(res: MsmResult) -> Dict:
    return {
        "c": res.c,
        "K": res.K,
        "rounds": res.rounds,
        "n_pairs": int(res.n_pairs),
        "n_pairs_algo": int(res.n_pairs_algo),
        "max_bucket": int(res.max_bucket),
        "tables": bool(res.tables),
        "phase_ms": {name: float(res.phase_ms[i]) for i, name in enumerate(_lib.PHASE_NAMES)},
    }


class MsmContext:
    """One curve bound to one GPU: thin object wrapper over the msm_* C functions."""

    def __init__(self, curve: int = _lib.CURVE_BLS12_377_G1, device: int = 0, devices: Optional[Sequence[int]] = None):
        """device: one GPU.  devices: a list of GPUs of this node -- the context then shards every MSM by scalar window
        across them from host threads inside the library (msm_ctx_create_multi)."""
        self._lib = _lib.load()
        h = C.c_void_p()
        if devices is not None and len(devices) > 0:
            arr = (C.c_int32 * len(devices))(*devices)
            rc = self._lib.msm_ctx_create_multi(C.byref(h), curve, arr, len(devices))
            device = devices[0]
        else:
            rc = self._lib.msm_ctx_create(C.byref(h), curve, device)
        if rc != _lib.MSM_OK:
            raise MsmError(rc, "msm_ctx_create failed (no usable GPU?) -- there is no CPU fallback")
        self._h = h
        self.curve = curve
        self.device = device
        self.n_points = 0
        self._cur_set = 0
        self._set_sizes: Dict[int, int] = {0: 0}
        self.coord_bytes = 32 if curve in _lib.CURVES_32_BYTE else 48   # per field, as the reference sizes them
        self._gen_buf, self._gen_cap = 0, 0   # device buffer of generate_scalars(into=0)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.msm_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc != _lib.MSM_OK:
            raise MsmError(rc, self._lib.msm_last_error(self._h).decode())

    # -- handles: point sets and device buffers ----------------------------------------------
    def pointset_create(self) -> int:
        """A new, empty resident point set; it becomes the current one (msm_pointset_create)."""
        i = C.c_int32()
        self._check(self._lib.msm_pointset_create(self._h, C.byref(i)))
        self.n_points = 0
        self._cur_set = i.value
        self._set_sizes[i.value] = 0
        return i.value

    def pointset_select(self, set_id: int) -> None:
        self._check(self._lib.msm_pointset_select(self._h, set_id))
        self._cur_set = set_id
        self.n_points = self._set_sizes.get(set_id, 0)

    def pointset_destroy(self, set_id: int) -> None:
        self._check(self._lib.msm_pointset_destroy(self._h, set_id))
        self._set_sizes.pop(set_id, None)
        if self._cur_set == set_id:
            self._cur_set = 0
            self.n_points = self._set_sizes.get(0, 0)

    def device_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self._lib.msm_device_alloc(self._h, nbytes, C.byref(p)))
        return int(p.value)

    def device_free(self, dev_ptr: int) -> None:
        self._check(self._lib.msm_device_free(self._h, C.c_void_p(dev_ptr)))

    def device_upload(self, dev_ptr: int, data: BytesLike) -> None:
        buf = data if isinstance(data, C.Array) else (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
        self._check(self._lib.msm_device_upload(self._h, C.c_void_p(dev_ptr), buf, len(data)))

    def set_workspace_limit(self, nbytes: int) -> None:
        """Device memory the working buffers of one call may take (0 = automatic); see include/msm_hip.h."""
        self._check(self._lib.msm_set_workspace_limit(self._h, int(nbytes)))

    @property
    def n_devices(self) -> int:
        return int(self._lib.msm_ctx_device_count(self._h))

    # -- points ---------------------------------------------------------------------------
    def set_points(self, points: BytesLike, check_curve: bool = False) -> int:
        step = 2 * self.coord_bytes
        if len(points) % step:
            raise MsmError(_lib.MSM_ERR_ARG, f"point buffer length {len(points)} is not a multiple of {step}")
        n = len(points) // step
        buf = (C.c_uint8 * max(len(points), 1)).from_buffer_copy(bytes(points) or b"\0")
        self._check(self._lib.msm_set_points(self._h, buf, n, 0, int(check_curve)))
        self.n_points = n
        self._set_sizes[self._cur_set] = n
        return n

    def set_points_device(self, dev_ptr: int, n: int, check_curve: bool = False) -> int:
        self._check(self._lib.msm_set_points(self._h, C.c_void_p(dev_ptr), n, 1, int(check_curve)))
        self.n_points = n
        self._set_sizes[self._cur_set] = n
        return n

    def generate_points(self, n: int, seed: int = 1, want_scalars: bool = False, raw: bool = False):
        """n resident points P_i = a_i G generated on the GPU.  want_scalars: also return the a_i (n x 32 bytes LE) --
        as `bytes`, or with raw=True as the ctypes array itself (no second 2 GB copy at 2^26)."""
        out = (C.c_uint8 * (32 * n))() if want_scalars and n else None
        self._check(self._lib.msm_generate_points(self._h, n, seed, out))
        self.n_points = n
        self._set_sizes[self._cur_set] = n
        if out is not None and raw:
            return out
        return bytes(out) if out is not None else (b"" if want_scalars else None)

    def generate_scalars(self, n: int, seed: int = 1, to_host: bool = False, into: int = 0, raw: bool = False):
        """n random scalars < q on the device.  `into`: caller-owned device pointer (n * 32 bytes); 0 = a device buffer this
        object allocates (msm_device_alloc) and keeps until the next such call or close().
        to_host: also return a host copy (bytes; the ctypes array itself with raw=True)."""
        if not into:
            if self._gen_buf and self._gen_cap < 32 * n:
                self.device_free(self._gen_buf)
                self._gen_buf = 0
            if not self._gen_buf:
                self._gen_buf, self._gen_cap = self.device_alloc(max(32 * n, 32)), max(32 * n, 32)
            into = self._gen_buf
        out = (C.c_uint8 * (32 * n))() if to_host and n else None
        self._check(self._lib.msm_generate_scalars(self._h, n, seed, C.c_void_p(into), out))
        if out is not None and raw:
            return int(into), out
        return int(into), (bytes(out) if out is not None else None)

    _VALIDATE = {None: _lib.VALIDATE_NONE, "none": _lib.VALIDATE_NONE, "curve": _lib.VALIDATE_CURVE,
                 "subgroup": _lib.VALIDATE_SUBGROUP}

    def _check_points(self, rc: int, bad: C.c_uint64) -> None:
        if rc != _lib.MSM_OK:
            idx = bad.value if bad.value != _lib.NO_BAD_INDEX else None
            raise MsmError(rc, self._lib.msm_last_error(self._h).decode(), bad_index=idx)

    def load_points(self, data: Union[BytesLike, int], *, compressed: bool = False, validate: Optional[str] = "subgroup",
                    on_device: bool = False, n: Optional[int] = None) -> int:
        """Resident points from x || y (compressed=False) or from the compressed encoding of the curve (include/msm_hip.h,
        INTEGRATION.md), validated at `validate`: "subgroup" (default: the curve equation and [q] P = O), "curve" or
        None / "none" (msm_set_points_ex).  on_device: `data` is a device pointer and `n` the number of points.
        A refused point raises MsmError(MSM_ERR_POINT) with its index in .bad_index; the point set is then empty."""
        if validate not in self._VALIDATE:
            raise MsmError(_lib.MSM_ERR_ARG, f"validate must be one of {sorted(k for k in self._VALIDATE if k)} or None")
        step = self.coord_bytes if compressed else 2 * self.coord_bytes
        if on_device:
            if n is None:
                raise MsmError(_lib.MSM_ERR_ARG, "load_points(on_device=True) needs n")
            ptr = C.c_void_p(int(data))
        else:
            if len(data) % step:
                raise MsmError(_lib.MSM_ERR_ARG, f"point buffer length {len(data)} is not a multiple of {step}")
            n = len(data) // step if n is None else n
            if n * step > len(data):
                raise MsmError(_lib.MSM_ERR_ARG, f"{n} points need {n * step} bytes, got {len(data)}")
            ptr = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
        bad = C.c_uint64()
        self.n_points = 0
        self._set_sizes[self._cur_set] = 0
        rc = self._lib.msm_set_points_ex(self._h, ptr, n, int(on_device),
                                         _lib.POINTS_COMPRESSED if compressed else _lib.POINTS_UNCOMPRESSED,
                                         self._VALIDATE[validate], C.byref(bad))
        self._check_points(rc, bad)
        self.n_points = n
        self._set_sizes[self._cur_set] = n
        return n

    def validate_points(self, first: int = 0, count: Optional[int] = None, level: Optional[str] = "subgroup") -> None:
        """Checks the resident points [first, first + count) (default: to the end) and changes nothing; raises MsmError with
        .bad_index at the first refused point (msm_validate_points)."""
        if level not in self._VALIDATE:
            raise MsmError(_lib.MSM_ERR_ARG, f"level must be one of {sorted(k for k in self._VALIDATE if k)} or None")
        count = self.n_points - first if count is None else count
        bad = C.c_uint64()
        self._check_points(self._lib.msm_validate_points(self._h, first, count, self._VALIDATE[level], C.byref(bad)), bad)

    def get_points(self, first: int, count: int, compressed: bool = False) -> bytes:
        """Resident points [first, first + count) as x || y, or compressed (the encoding load_points(compressed=True) reads)."""
        step = self.coord_bytes if compressed else 2 * self.coord_bytes
        out = (C.c_uint8 * max(step * count, 1))()
        if compressed:
            self._check(self._lib.msm_get_points_ex(self._h, first, count, _lib.POINTS_COMPRESSED, out))
        else:
            self._check(self._lib.msm_get_points(self._h, first, count, out))
        return bytes(out)[: step * count]

    def get_point(self, i: int) -> Optional[Tuple[int, int]]:
        b = self.get_points(i, 1)
        nb = self.coord_bytes
        x, y = int.from_bytes(b[:nb], "little"), int.from_bytes(b[nb:], "little")
        return None if (x == 0 and y == 0) else (x, y)

    # -- msm ------------------------------------------------------------------------------
    def plan(self, n: int, c: Optional[int] = None, no_tables: bool = False, merged: bool = False, point_lo: int = 0) -> Tuple[int, int]:
        """(c, K) of msm_run over n points; over the whole resident point set that is the plan on window tables where they
        exist or would be built -- no_tables: the plain plan (what msm_window_sums without `merged` and bucket shards run);
        merged: the plan of window_sums(..., merged=True), and of run_device, over the points [point_lo, point_lo + n), which may
        run on the window tables of that range.  It is the (c, K) the very next such call reports and every one after it, whether
        the tables exist yet or not (the call before the build runs the plain path under the tables' window); only new points,
        set_tables_limit, precompute or tables of the whole set replacing a range's move it."""
        opts = MsmOpts(c=c or 0, no_tables=int(no_tables), merged_sums=int(merged), point_lo=point_lo)
        cc, kk = C.c_int32(), C.c_int32()
        self._check(self._lib.msm_plan(self._h, n, C.byref(opts), C.byref(cc), C.byref(kk)))
        return cc.value, kk.value

    def run(self, scalars: BytesLike, c: Optional[int] = None, unsafe: bool = False, no_glv: bool = False,
            by_window: bool = False, no_tables: bool = False) -> Tuple[AffineResult, Dict]:
        if len(scalars) % 32:
            raise MsmError(_lib.MSM_ERR_ARG, f"scalar buffer length {len(scalars)} is not a multiple of 32")
        n = len(scalars) // 32
        # a ctypes array is handed over as it is (no 2 GB copies at 2^26), anything else is copied once
        buf = scalars if isinstance(scalars, C.Array) else (C.c_uint8 * max(len(scalars), 1)).from_buffer_copy(bytes(scalars) or b"\0")
        return self._run(buf, n, 0, c, unsafe, no_glv=no_glv, by_window=by_window, no_tables=no_tables)

    def run_device(self, dev_ptr: int, n: int, c: Optional[int] = None, unsafe: bool = False, serial: bool = False,
                   no_glv: bool = False, by_window: bool = False, point_lo: int = 0, no_tables: bool = False) -> Tuple[AffineResult, Dict]:
        """by_window: a device-list context shards by scalar window instead of by points.  point_lo: the MSM covers the
        resident points [point_lo, point_lo + n) (scalar i belongs to point point_lo + i).  no_tables: the plain path even
        where window tables exist or would be built (msm_opts.no_tables)."""
        return self._run(C.c_void_p(dev_ptr), n, 1, c, unsafe, serial, no_glv, by_window, point_lo, no_tables)

    def run_placed(self, dev_ptrs: Sequence[int], n: int, c: Optional[int] = None) -> Tuple[AffineResult, Dict]:
        """Device-list context, scalars already placed: dev_ptrs[d] on devices[d] holds the scalars of that device's share
        [n d / G, n (d + 1) / G) of the points (msm_run_placed)."""
        arr = (C.c_void_p * len(dev_ptrs))(*[C.c_void_p(int(p)) for p in dev_ptrs])
        opts, res = MsmOpts(c=c or 0), MsmResult()
        self._check(self._lib.msm_run_placed(self._h, arr, n, C.byref(opts), C.byref(res)))
        nb = self.coord_bytes
        out = AffineResult(int.from_bytes(bytes(res.x)[:nb], "little"), int.from_bytes(bytes(res.y)[:nb], "little"),
                           bool(res.is_infinity))
        return out, _result_to_dict(res)

    def _run(self, ptr, n: int, on_device: int, c: Optional[int], unsafe: bool, serial: bool = False,
             no_glv: bool = False, by_window: bool = False, point_lo: int = 0, no_tables: bool = False) -> Tuple[AffineResult, Dict]:
        opts = MsmOpts(c=c or 0, unsafe=int(unsafe), serial=int(serial), no_glv=int(no_glv), by_window=int(by_window),
                       point_lo=point_lo, no_tables=int(no_tables))
        res = MsmResult()
        self._check(self._lib.msm_run(self._h, ptr, n, on_device, C.byref(opts), C.byref(res)))
        nb = self.coord_bytes
        out = AffineResult(
            x=int.from_bytes(bytes(res.x)[:nb], "little"),
            y=int.from_bytes(bytes(res.y)[:nb], "little"),
            isZero=bool(res.is_infinity),
        )
        return out, _result_to_dict(res)

    def run_batch(self, scalars: Sequence[BytesLike], c: Optional[int] = None, unsafe: bool = False, no_glv: bool = False,
                  strict: bool = False, serial: bool = False, point_lo: int = 0,
                  no_tables: bool = False) -> List[Tuple[AffineResult, Dict]]:
        """B MSMs over the same resident points (msm_run_batch): scalars[b] is the n x 32-byte scalar vector of element b, all
        of the same length.  Element b equals run(scalars[b]); the info dicts describe the whole batched call."""
        if not scalars:
            raise MsmError(_lib.MSM_ERR_ARG, "run_batch: empty batch")
        n = len(scalars[0]) // 32
        bufs = []
        for s in scalars:
            if len(s) != 32 * n or len(s) % 32:
                raise MsmError(_lib.MSM_ERR_ARG, "run_batch: the scalar vectors must all be n x 32 bytes")
            bufs.append(s if isinstance(s, C.Array) else (C.c_uint8 * max(len(s), 1)).from_buffer_copy(bytes(s) or b"\0"))
        ptrs = [C.cast(b, C.c_void_p).value for b in bufs]
        return self._run_batch(ptrs, n, 0, c, unsafe, no_glv, strict, serial, point_lo, no_tables)

    def run_batch_device(self, dev_ptrs: Sequence[int], n: int, c: Optional[int] = None, unsafe: bool = False,
                         no_glv: bool = False, strict: bool = False, serial: bool = False, point_lo: int = 0,
                         no_tables: bool = False) -> List[Tuple[AffineResult, Dict]]:
        """run_batch over device scalar buffers (n x 32 bytes each, e.g. from device_alloc)."""
        return self._run_batch([int(p) for p in dev_ptrs], n, 1, c, unsafe, no_glv, strict, serial, point_lo, no_tables)

    def _run_batch(self, ptrs: Sequence[int], n: int, on_device: int, c, unsafe, no_glv, strict, serial, point_lo,
                   no_tables) -> List[Tuple[AffineResult, Dict]]:
        B = len(ptrs)
        arr = (C.c_void_p * max(B, 1))(*[C.c_void_p(p) for p in ptrs])
        opts = MsmOpts(c=c or 0, unsafe=int(unsafe), serial=int(serial), no_glv=int(no_glv), strict=int(strict),
                       point_lo=point_lo, no_tables=int(no_tables))
        res = (MsmResult * max(B, 1))()
        self._check(self._lib.msm_run_batch(self._h, arr, B, n, on_device, C.byref(opts), res))
        nb = self.coord_bytes
        return [(AffineResult(int.from_bytes(bytes(r.x)[:nb], "little"), int.from_bytes(bytes(r.y)[:nb], "little"),
                              bool(r.is_infinity)), _result_to_dict(r)) for r in res[:B]]

    # -- narrow scalars (msm_run_narrow, include/msm_hip.h) -----------------------------------
    def _narrow_buffer(self, scalars, width: Optional[int], signed: Optional[bool]):
        """(ctypes buffer, n, width, signed) of a numpy array (format from its dtype) or of bytes with width=."""
        from . import narrow as N

        if hasattr(scalars, "dtype"):
            import numpy as np

            w, s = N.dtype_format(scalars.dtype)
            if width not in (None, w) or signed not in (None, s):
                raise MsmError(_lib.MSM_ERR_ARG, f"width / signed contradict the array's dtype {scalars.dtype}")
            raw = np.ascontiguousarray(scalars).tobytes()
            width, signed = w, s
        else:
            if width is None:
                raise MsmError(_lib.MSM_ERR_ARG, "narrow scalars given as bytes need width=")
            raw = bytes(scalars)
            signed = bool(signed)
        if width <= 0 or len(raw) % width:
            raise MsmError(_lib.MSM_ERR_ARG, f"scalar buffer length {len(raw)} is not a multiple of the width {width}")
        return (C.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw or b"\0"), len(raw) // width, width, bool(signed)

    def run_narrow(self, scalars, bits: Optional[int] = None, signed: Optional[bool] = None, c: Optional[int] = None,
                   point_lo: int = 0, serial: bool = False, width: Optional[int] = None) -> Tuple[AffineResult, Dict]:
        """MSM over narrow scalars (msm_run_narrow): a numpy array of dtype uint8/16/32/64 or int8/16/32/64 (width and
        signedness from the dtype), or bytes with width= (1, 2, 4, 8, 16, or 32 for field elements holding small values).
        bits: magnitude bits, default all the width gives; values in [0, 2^bits), signed [-2^bits, 2^bits).  Equal to run()
        over the same values widened to 32 bytes (montgomery_amd.narrow.widen); a value outside the range raises
        MsmError(MSM_ERR_SCALAR)."""
        buf, n, width, signed = self._narrow_buffer(scalars, width, signed)
        return self._run_narrow(buf, n, 0, width, bits, signed, c, point_lo, serial)

    def run_narrow_device(self, dev_ptr: int, n: int, width: int, bits: Optional[int] = None, signed: bool = False,
                          c: Optional[int] = None, point_lo: int = 0, serial: bool = False) -> Tuple[AffineResult, Dict]:
        """run_narrow over a device buffer of n x width bytes."""
        return self._run_narrow(C.c_void_p(dev_ptr), n, 1, width, bits, signed, c, point_lo, serial)

    def _run_narrow(self, ptr, n, on_device, width, bits, signed, c, point_lo, serial) -> Tuple[AffineResult, Dict]:
        opts, res = MsmOpts(c=c or 0, serial=int(serial), point_lo=point_lo), MsmResult()
        self._check(self._lib.msm_run_narrow(self._h, ptr, n, on_device, width, bits or 0, int(bool(signed)), C.byref(opts),
                                             C.byref(res)))
        nb = self.coord_bytes
        return (AffineResult(int.from_bytes(bytes(res.x)[:nb], "little"), int.from_bytes(bytes(res.y)[:nb], "little"),
                             bool(res.is_infinity)), _result_to_dict(res))

    def run_batch_narrow(self, scalars: Sequence, bits: Optional[int] = None, signed: Optional[bool] = None,
                         c: Optional[int] = None, point_lo: int = 0, serial: bool = False,
                         width: Optional[int] = None) -> List[Tuple[AffineResult, Dict]]:
        """B narrow MSMs over the same resident points (msm_run_batch_narrow): one array (or bytes with width=) per element,
        all of one format and length.  Element b equals run_narrow(scalars[b])."""
        if not len(scalars):
            raise MsmError(_lib.MSM_ERR_ARG, "run_batch_narrow: empty batch")
        bufs = [self._narrow_buffer(s, width, signed) for s in scalars]
        if any(b[1:] != bufs[0][1:] for b in bufs):
            raise MsmError(_lib.MSM_ERR_ARG, "run_batch_narrow: the elements must share one format and length")
        _, n, w, sg = bufs[0]
        ptrs = [C.cast(b[0], C.c_void_p).value for b in bufs]
        return self._run_batch_narrow(ptrs, n, 0, w, bits, sg, c, point_lo, serial)

    def run_batch_narrow_device(self, dev_ptrs: Sequence[int], n: int, width: int, bits: Optional[int] = None,
                                signed: bool = False, c: Optional[int] = None, point_lo: int = 0,
                                serial: bool = False) -> List[Tuple[AffineResult, Dict]]:
        """run_batch_narrow over device buffers of n x width bytes each."""
        return self._run_batch_narrow([int(p) for p in dev_ptrs], n, 1, width, bits, signed, c, point_lo, serial)

    def _run_batch_narrow(self, ptrs, n, on_device, width, bits, signed, c, point_lo, serial):
        B = len(ptrs)
        arr = (C.c_void_p * max(B, 1))(*[C.c_void_p(p) for p in ptrs])
        opts = MsmOpts(c=c or 0, serial=int(serial), point_lo=point_lo)
        res = (MsmResult * max(B, 1))()
        self._check(self._lib.msm_run_batch_narrow(self._h, arr, B, n, on_device, width, bits or 0, int(bool(signed)),
                                                   C.byref(opts), res))
        nb = self.coord_bytes
        return [(AffineResult(int.from_bytes(bytes(r.x)[:nb], "little"), int.from_bytes(bytes(r.y)[:nb], "little"),
                              bool(r.is_infinity)), _result_to_dict(r)) for r in res[:B]]

    def plan_narrow(self, n: int, bits: int, c: Optional[int] = None) -> Tuple[int, int]:
        """(c, K) of run_narrow over n points and scalars of `bits` magnitude bits (msm_plan_narrow)."""
        opts = MsmOpts(c=c or 0)
        cc, kk = C.c_int32(), C.c_int32()
        self._check(self._lib.msm_plan_narrow(self._h, n, bits, C.byref(opts), C.byref(cc), C.byref(kk)))
        return cc.value, kk.value

    def scalar_bits(self, scalars: Union[BytesLike, int], n: Optional[int] = None) -> Tuple[int, int]:
        """(unsigned, signed) magnitude bits of n x 32-byte scalars -- host bytes, or a device pointer with n=: the smallest
        `bits` run_narrow(width=32) accepts them under (0: all zero; 255: a scalar needs more than 128 bits)."""
        if isinstance(scalars, int):
            if n is None:
                raise MsmError(_lib.MSM_ERR_ARG, "scalar_bits over a device pointer needs n")
            ptr, on_device = C.c_void_p(scalars), 1
        else:
            if len(scalars) % 32:
                raise MsmError(_lib.MSM_ERR_ARG, f"scalar buffer length {len(scalars)} is not a multiple of 32")
            n = len(scalars) // 32 if n is None else n
            ptr = scalars if isinstance(scalars, C.Array) else (C.c_uint8 * max(len(scalars), 1)).from_buffer_copy(bytes(scalars) or b"\0")
            on_device = 0
        ub, sb = C.c_int32(), C.c_int32()
        self._check(self._lib.msm_scalar_bits(self._h, ptr, n, on_device, C.byref(ub), C.byref(sb)))
        return ub.value, sb.value

    # -- indexed (sparse) MSM (msm_run_indexed, include/msm_hip.h) -----------------------------
    def _affine(self, res: MsmResult) -> AffineResult:
        nb = self.coord_bytes
        return AffineResult(int.from_bytes(bytes(res.x)[:nb], "little"), int.from_bytes(bytes(res.y)[:nb], "little"),
                            bool(res.is_infinity))

    def msm_indexed(self, scalars, indices, *, c: Optional[int] = None, no_glv: bool = False, strict: bool = False,
                    serial: bool = False) -> Tuple[AffineResult, Dict]:
        """sum_j scalars[j] * P[indices[j]] over the current point set (msm_run_indexed): scalars as bytes of m x 32 (or a
        uint8 numpy array / torch tensor of shape (m, 32)), indices as a 1-d integer array / tensor or a sequence of ints, in
        any order and with repeats.  Equal to run() over the dense equivalent (dense_from_sparse); the window is picked for m.
        An index >= the resident count raises MsmError(MSM_ERR_ARG) naming its position."""
        raw = _wide_scalar_bytes(scalars)
        idx = _index_array(indices, len(raw) // 32)
        sbuf = (C.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
        return self._run_indexed(sbuf, idx.ctypes.data_as(C.POINTER(C.c_uint32)), idx.size, 0, c, no_glv, strict, serial)

    def msm_indexed_device(self, dev_scalars: int, dev_indices: int, m: int, *, c: Optional[int] = None, no_glv: bool = False,
                           strict: bool = False, serial: bool = False) -> Tuple[AffineResult, Dict]:
        """msm_indexed over device buffers: m x 32 bytes of scalars and m uint32 indices (4-byte aligned)."""
        return self._run_indexed(C.c_void_p(dev_scalars), C.cast(C.c_void_p(dev_indices), C.POINTER(C.c_uint32)), m, 1, c, no_glv,
                                 strict, serial)

    def _run_indexed(self, sptr, iptr, m, on_device, c, no_glv, strict, serial) -> Tuple[AffineResult, Dict]:
        opts, res = MsmOpts(c=c or 0, no_glv=int(no_glv), strict=int(strict), serial=int(serial)), MsmResult()
        self._check(self._lib.msm_run_indexed(self._h, sptr, iptr, m, on_device, C.byref(opts), C.byref(res)))
        return self._affine(res), _result_to_dict(res)

    def msm_indexed_narrow(self, scalars, indices, *, bits: Optional[int] = None, signed: Optional[bool] = None,
                           c: Optional[int] = None, serial: bool = False, width: Optional[int] = None) -> Tuple[AffineResult, Dict]:
        """msm_indexed over narrow scalars (msm_run_indexed_narrow): scalars, bits, signed and width as for run_narrow."""
        buf, m, width, signed = self._narrow_buffer(_as_numpy(scalars), width, signed)
        idx = _index_array(indices, m)
        return self._run_indexed_narrow(buf, idx.ctypes.data_as(C.POINTER(C.c_uint32)), m, 0, width, bits, signed, c, serial)

    def msm_indexed_narrow_device(self, dev_scalars: int, dev_indices: int, m: int, width: int, *, bits: Optional[int] = None,
                                  signed: bool = False, c: Optional[int] = None, serial: bool = False) -> Tuple[AffineResult, Dict]:
        """msm_indexed_narrow over device buffers: m x width bytes of scalars and m uint32 indices."""
        return self._run_indexed_narrow(C.c_void_p(dev_scalars), C.cast(C.c_void_p(dev_indices), C.POINTER(C.c_uint32)), m, 1, width,
                                        bits, signed, c, serial)

    def _run_indexed_narrow(self, sptr, iptr, m, on_device, width, bits, signed, c, serial) -> Tuple[AffineResult, Dict]:
        opts, res = MsmOpts(c=c or 0, serial=int(serial)), MsmResult()
        self._check(self._lib.msm_run_indexed_narrow(self._h, sptr, iptr, m, on_device, width, bits or 0, int(bool(signed)),
                                                     C.byref(opts), C.byref(res)))
        return self._affine(res), _result_to_dict(res)

    # -- point-set linear combinations (msm_points_lincomb, include/msm_hip.h) -----------------
    def pointset_size(self, set_id: Optional[int] = None) -> int:
        """Resident points of a point set (default: the current one), as the library counts them (msm_pointset_size)."""
        n = C.c_uint64()
        self._check(self._lib.msm_pointset_size(self._h, self._cur_set if set_id is None else set_id, C.byref(n)))
        return int(n.value)

    def points_lincomb(self, a, b=None, *, src_a: Optional[int] = None, a_lo: int = 0, src_b: Optional[int] = None, b_lo: int = 0,
                       count: Optional[int] = None, dst: Optional[int] = None) -> int:
        """D[i] = a * A[a_lo + i] + b * B[b_lo + i], i < count, as the rows [0, count) of point set `dst`, which then holds
        `count` points (msm_points_lincomb).  a, b: ints or 32 little-endian bytes, < q; b None: no second term.  src_a, src_b,
        dst: point-set ids, default the current set; count: default all of A from a_lo on.  dst may be a source (see
        include/msm_hip.h for the overlaps allowed); the current set stays selected.  Returns count."""
        sa = _scalar32(a, "a")
        sb = None if b is None else _scalar32(b, "b")
        if a_lo < 0 or b_lo < 0 or (count is not None and count < 0):
            raise MsmError(_lib.MSM_ERR_ARG, "points_lincomb: a_lo, b_lo and count must not be negative")
        cur = self._cur_set
        ia = cur if src_a is None else src_a
        ib = -1 if sb is None else (cur if src_b is None else src_b)
        idst = cur if dst is None else dst
        if count is None:
            count = max(self.pointset_size(ia) - a_lo, 0)
        abuf = (C.c_uint8 * 32).from_buffer_copy(sa)
        bbuf = (C.c_uint8 * 32).from_buffer_copy(sb) if sb is not None else None
        self._check(self._lib.msm_points_lincomb(self._h, ia, a_lo, abuf, ib, b_lo, bbuf, count, idst))
        self._set_sizes[idst] = count
        if idst == cur:
            self.n_points = count
        return count

    def fold_points(self, lo_scalar, hi_scalar) -> int:
        """The in-place fold of the current set: P[i] <- lo_scalar * P[i] + hi_scalar * P[i + n/2], i < n/2 (n even); the set
        shrinks to n/2 points and loses its window tables.  The generator fold of an inner-product argument: (1, u) in Halo2,
        (u^-1, u) in Bulletproofs.  Returns n/2."""
        sa, sb = _scalar32(lo_scalar, "lo_scalar"), _scalar32(hi_scalar, "hi_scalar")
        n = self.n_points
        if n % 2:
            raise MsmError(_lib.MSM_ERR_ARG, f"fold_points: the set holds {n} points, an odd number")
        return self.points_lincomb(sa, sb, a_lo=0, b_lo=n // 2, count=n // 2)

    # -- per-row scalar multiplication (msm_points_mul, msm_points_mul_base, include/msm_hip.h) ---
    @staticmethod
    def _scalar_vector(scalars, count: Optional[int], who: str):
        """(pointer argument, on_device, count, keep-alive) of a vector of 32-byte scalars: an int is a device address (count is
        then required), anything else n x 32 host bytes (bytes, bytearray, a ctypes or numpy array), as run() takes them."""
        if isinstance(scalars, bool) or scalars is None:
            raise MsmError(_lib.MSM_ERR_ARG, f"{who}: scalars must be bytes, an array or a device address")
        if count is not None and count < 0:
            raise MsmError(_lib.MSM_ERR_ARG, f"{who}: count must not be negative")
        if isinstance(scalars, int):
            if count is None:
                raise MsmError(_lib.MSM_ERR_ARG, f"{who}: a device address needs count")
            return C.c_void_p(scalars), 1, count, None
        if not isinstance(scalars, (bytes, bytearray, memoryview, C.Array)):
            scalars = _as_numpy(scalars).tobytes()
        if len(scalars) % 32:
            raise MsmError(_lib.MSM_ERR_ARG, f"{who}: scalar buffer length {len(scalars)} is not a multiple of 32")
        n = len(scalars) // 32
        if count is None:
            count = n
        if count > n:
            raise MsmError(_lib.MSM_ERR_ARG, f"{who}: count {count} exceeds the {n} scalars given")
        buf = scalars if isinstance(scalars, C.Array) else (C.c_uint8 * max(len(scalars), 1)).from_buffer_copy(bytes(scalars) or b"\0")
        return buf, 0, count, buf

    def _points_written(self, idst: int, count: int) -> int:
        self._set_sizes[idst] = count
        if idst == self._cur_set:
            self.n_points = count
        return count

    def points_mul(self, scalars, *, src: Optional[int] = None, a_lo: int = 0, count: Optional[int] = None,
                   dst: Optional[int] = None) -> int:
        """D[i] = s[i] * A[a_lo + i], i < count, as the rows [0, count) of point set `dst` (msm_points_mul): every row under its
        own scalar.  scalars: n x 32 little-endian bytes (bytes, bytearray, an array) or a device address (16-byte aligned, e.g.
        what scalars_powers wrote; count is then required); values >= q are reduced.  src, dst: point-set ids, default the
        current set; count: default the number of host scalars.  dst may be src with a_lo == 0 or a_lo >= count.  Returns count."""
        if a_lo < 0:
            raise MsmError(_lib.MSM_ERR_ARG, "points_mul: a_lo must not be negative")
        ptr, on_device, count, _keep = self._scalar_vector(scalars, count, "points_mul")
        cur = self._cur_set
        isrc, idst = cur if src is None else src, cur if dst is None else dst
        self._check(self._lib.msm_points_mul(self._h, isrc, a_lo, ptr, on_device, count, idst))
        return self._points_written(idst, count)

    def points_mul_base(self, scalars, base=None, *, count: Optional[int] = None, dst: Optional[int] = None) -> int:
        """D[i] = s[i] * P, i < count, as the rows [0, count) of point set `dst` (msm_points_mul_base).  base: x || y in the wire
        format of set_points (bytes), or None for the curve's generator; the all-zero encoding is the identity.  scalars, count,
        dst: as points_mul.  The context caches the table of the last base.  Returns count."""
        if base is not None:
            base = bytes(base)
            if len(base) != 2 * self.coord_bytes:
                raise MsmError(_lib.MSM_ERR_ARG, f"points_mul_base: the base must be {2 * self.coord_bytes} bytes (x || y)")
        ptr, on_device, count, _keep = self._scalar_vector(scalars, count, "points_mul_base")
        idst = self._cur_set if dst is None else dst
        bbuf = None if base is None else (C.c_uint8 * len(base)).from_buffer_copy(base)
        self._check(self._lib.msm_points_mul_base(self._h, bbuf, ptr, on_device, count, idst))
        return self._points_written(idst, count)

    # -- the transform over point sets (msm_points_ntt, include/msm_hip.h) ----------------------
    def points_ntt(self, *, src: Optional[int] = None, a_lo: int = 0, log2n: int, omega=None, shift=None, inverse: bool = False,
                   dst: Optional[int] = None) -> int:
        """The number-theoretic transform over the n = 2^log2n rows [a_lo, a_lo + n) of point set `src`, written as the rows
        [0, n) of point set `dst` (msm_points_ntt).  forward: D[k] = sum_j (shift omega^k)^j A[j]; inverse: the exact inverse map
        (n^-1 and shift^-j included): over a monomial key [tau^j] G and without a shift it gives the key in the Lagrange basis of
        <omega> (the key of a coset: include/msm_hip.h).  omega: a primitive n-th root of unity < q (int or 32 bytes), None = scalars_root_of_unity(log2n); shift: in
        [1, q), None = 1.  src, dst: point-set ids, default the current set; dst may be src with a_lo == 0 or a_lo >= n.
        Returns n."""
        if a_lo < 0 or log2n < 0:
            raise MsmError(_lib.MSM_ERR_ARG, "points_ntt: a_lo and log2n must not be negative")
        om = None if omega is None else self._scalar_buf(omega, "omega")
        sh = None if shift is None else self._scalar_buf(shift, "shift")
        cur = self._cur_set
        isrc, idst = cur if src is None else src, cur if dst is None else dst
        self._check(self._lib.msm_points_ntt(self._h, isrc, a_lo, log2n, om, sh, int(bool(inverse)), idst))
        return self._points_written(idst, 1 << log2n)

    # -- resident scalar-vector operations (msm_scalars_*, include/msm_hip.h) -------------------
    def device_download(self, dev_ptr: int, nbytes: int) -> bytes:
        """`nbytes` bytes of device memory, from a buffer of device_alloc or any device address (msm_device_download)."""
        buf = (C.c_uint8 * max(nbytes, 1))()
        self._check(self._lib.msm_device_download(self._h, buf, C.c_void_p(dev_ptr), nbytes))
        return bytes(buf[:nbytes])

    @staticmethod
    def _scalar_buf(v, what: str):
        return (C.c_uint8 * 32).from_buffer_copy(_scalar32(v, what))

    def scalars_lincomb(self, dst: int, x, a: int, y=None, b: Optional[int] = None, n: int = 0) -> None:
        """dst[i] = x * a[i] + y * b[i] mod q, i < n, over vectors of 32-byte scalars in device memory (msm_scalars_lincomb).
        dst, a, b: device addresses (16-byte aligned); x, y: ints or 32 little-endian bytes, < q.  y and b None: one term.
        dst may be a or b themselves, or disjoint from both."""
        if (y is None) != (b is None):
            raise MsmError(_lib.MSM_ERR_ARG, "scalars_lincomb: y and b come together")
        ybuf = None if y is None else self._scalar_buf(y, "y")
        self._check(self._lib.msm_scalars_lincomb(self._h, C.c_void_p(dst), self._scalar_buf(x, "x"), C.c_void_p(a), ybuf,
                                                  None if b is None else C.c_void_p(b), n))

    def scalars_mul(self, dst: int, a: int, b: int, n: int) -> None:
        """dst[i] = a[i] * b[i] mod q (msm_scalars_mul)."""
        self._check(self._lib.msm_scalars_mul(self._h, C.c_void_p(dst), C.c_void_p(a), C.c_void_p(b), n))

    def scalars_inner(self, a: int, b: int, n: int) -> int:
        """sum_i a[i] * b[i] mod q as an int (msm_scalars_inner); 0 for n == 0."""
        out = (C.c_uint8 * 32)()
        self._check(self._lib.msm_scalars_inner(self._h, C.c_void_p(a), C.c_void_p(b), n, out))
        return int.from_bytes(bytes(out), "little")

    def scalars_powers(self, dst: int, x, n: int, s=1) -> None:
        """dst[i] = s * x^i mod q, i < n (msm_scalars_powers)."""
        self._check(self._lib.msm_scalars_powers(self._h, C.c_void_p(dst), self._scalar_buf(s, "s"), self._scalar_buf(x, "x"), n))

    def scalars_ntt(self, dst: int, a: int, log2n: int, inverse: bool = False, omega=None, shift=None, batch: int = 1) -> None:
        """`batch` transforms of n = 2^log2n scalars each, vectors back to back, natural order in and out (msm_scalars_ntt).
        forward: dst[k] = sum_j a[j] (shift omega^k)^j; inverse: the exact inverse map (n^-1 and shift^-j included).
        omega: a primitive n-th root of unity < q (int or 32 bytes), None = scalars_root_of_unity(log2n); shift: in [1, q),
        None = 1.  dst may be a itself or disjoint from it."""
        om = None if omega is None else self._scalar_buf(omega, "omega")
        sh = None if shift is None else self._scalar_buf(shift, "shift")
        self._check(self._lib.msm_scalars_ntt(self._h, C.c_void_p(dst), C.c_void_p(a), log2n, batch, om, sh, int(bool(inverse))))

    def scalars_root_of_unity(self, log2n: int) -> int:
        """The library's primitive 2^log2n-th root of unity mod q as an int: g^((q-1)/2^log2n), g the smallest non-residue."""
        out = (C.c_uint8 * 32)()
        rc = self._lib.msm_scalars_root_of_unity(self._h, log2n, out)
        if rc:
            raise MsmError(rc, f"scalars_root_of_unity: q - 1 has no factor 2^{log2n}")
        return int.from_bytes(bytes(out), "little")

    def scalars_ntt_max_log2n(self) -> int:
        """The largest log2n scalars_ntt accepts on this context: min(two-adicity of q - 1, 29)."""
        out = C.c_uint32(0)
        self._check(self._lib.msm_scalars_ntt_max_log2n(self._h, C.byref(out)))
        return int(out.value)

    def scalars_scan(self, dst: int, a: int, n: int, op: str = "sum", exclusive: bool = False, init=None) -> int:
        """The running sum (op "sum") or product ("product") mod q of the n scalars at a (msm_scalars_scan):
        inclusive dst[i] = init o a[0] o ... o a[i]; exclusive dst[i] = init o a[0] o ... o a[i-1].  init: int or 32 bytes < q,
        None = 0 / 1.  dst may be a itself or disjoint from it.  Returns the total init o a[0] o ... o a[n-1] as an int."""
        ops = {"sum": _lib.SCAN_SUM, "product": _lib.SCAN_PRODUCT}
        if op not in ops:
            raise MsmError(_lib.MSM_ERR_ARG, f"scalars_scan: op must be 'sum' or 'product', not {op!r}")
        out = (C.c_uint8 * 32)()
        ibuf = None if init is None else self._scalar_buf(init, "init")
        self._check(self._lib.msm_scalars_scan(self._h, C.c_void_p(dst), C.c_void_p(a), n, ops[op],
                                               _lib.SCAN_EXCLUSIVE if exclusive else 0, ibuf, out))
        return int.from_bytes(bytes(out), "little")

    def scalars_inverse(self, dst: int, a: int, n: int) -> int:
        """dst[i] = a[i]^-1 mod q; an element whose residue is 0 gives 0 (msm_scalars_inverse).  dst may be a itself or disjoint
        from it.  Returns how many elements had the residue 0."""
        zeros = C.c_uint64(0)
        self._check(self._lib.msm_scalars_inverse(self._h, C.c_void_p(dst), C.c_void_p(a), n, C.byref(zeros)))
        return int(zeros.value)

    def scalars_div_linear(self, dst: int, a: int, n: int, z) -> int:
        """The division of the polynomial with the n coefficients at a (a[0] the constant term) by X - z (msm_scalars_div_linear):
        dst[j] = q_j for j < n - 1 and dst[n-1] = 0, where a(X) = (X - z) q(X) + a(z).  z: int or 32 bytes < q.  dst may be a itself
        or disjoint from it.  Returns the remainder a(z) as an int."""
        out = (C.c_uint8 * 32)()
        self._check(self._lib.msm_scalars_div_linear(self._h, C.c_void_p(dst), C.c_void_p(a), n, self._scalar_buf(z, "z"), out))
        return int.from_bytes(bytes(out), "little")

    @staticmethod
    def _ptr_array(ptrs, what: str):
        ptrs = list(ptrs)
        if not ptrs:
            raise MsmError(_lib.MSM_ERR_ARG, f"{what}: no vectors")
        return (C.c_void_p * len(ptrs))(*[int(p) for p in ptrs]), len(ptrs)

    def scalars_sumcheck_round(self, vecs, log2n: int, var: int, shape: str = "prod") -> List[int]:
        """The round polynomial of a sumcheck over the multilinear tables at the device addresses `vecs`, 2^log2n scalars each
        (msm_scalars_sumcheck_round): s(t) = sum over the pairs i of g(f_0(i, t), ..), f_j(i, t) = a_j[lo(i)] + t (a_j[hi(i)] -
        a_j[lo(i)]), as ints for t = 0 .. d.  Variable `var` is bit `var` of the index (0 = least significant).  shape "prod":
        g = the product of 1 .. 4 tables, d = their number; "r1cs": g = f_0 (f_1 f_2 - f_3), four tables, d = 3.  s(0) + s(1)
        is the claim of the round.  A sum of products runs one call per product: the round polynomial is linear in g."""
        shapes = {"prod": _lib.SUMCHECK_PROD, "r1cs": _lib.SUMCHECK_R1CS}
        if shape not in shapes:
            raise MsmError(_lib.MSM_ERR_ARG, f"scalars_sumcheck_round: shape must be 'prod' or 'r1cs', not {shape!r}")
        arr, m = self._ptr_array(vecs, "scalars_sumcheck_round")
        out = (C.c_uint8 * (32 * 5))()
        self._check(self._lib.msm_scalars_sumcheck_round(self._h, arr, m, log2n, var, shapes[shape], out))
        d = 3 if shape == "r1cs" else m
        raw = bytes(out)
        return [int.from_bytes(raw[32 * t:32 * t + 32], "little") for t in range(d + 1)]

    def scalars_bind(self, dst, a, log2n: int, var: int, r) -> None:
        """Binds variable `var` of the tables at the device addresses `a` (1 .. 8 of them, 2^log2n scalars each) to r, into the
        addresses `dst` (msm_scalars_bind): dst_j[i] = a_j[lo(i)] + r (a_j[hi(i)] - a_j[lo(i)]), i < 2^(log2n - 1).  dst and a:
        one address or a sequence of as many.  dst_j may be a_j itself when var is the top variable (the upper half then stays
        as it was); every other overlap of a destination is refused.  r: int or 32 bytes < q."""
        dst = [dst] if isinstance(dst, int) else list(dst)
        a = [a] if isinstance(a, int) else list(a)
        if len(dst) != len(a):
            raise MsmError(_lib.MSM_ERR_ARG, f"scalars_bind: {len(dst)} destinations for {len(a)} tables")
        darr, m = self._ptr_array(dst, "scalars_bind")
        aarr, _ = self._ptr_array(a, "scalars_bind")
        self._check(self._lib.msm_scalars_bind(self._h, darr, aarr, m, log2n, var, self._scalar_buf(r, "r")))

    def scalars_eq(self, dst: int, r, s=None) -> None:
        """dst[i] = s * prod_j (bit_j(i) ? r[j] : 1 - r[j]) mod q for i < 2^len(r): the table eq(r, .) scaled by s
        (msm_scalars_eq).  r: a sequence of ints or 32-byte strings < q, entry j belonging to bit j of the index; s: None = 1."""
        r = list(r)
        raw = b"".join(_scalar32(x, "an entry of r") for x in r)
        rbuf = (C.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
        sbuf = None if s is None else self._scalar_buf(s, "s")
        self._check(self._lib.msm_scalars_eq(self._h, C.c_void_p(dst), rbuf, len(r), sbuf))

    # -- resident sparse matrices (msm_matrix_*, msm_scalars_matvec) ---------------------------
    @staticmethod
    def _u32_buf(a, what: str):
        """host uint32 array from a sequence of ints, a numpy array or little-endian bytes"""
        if isinstance(a, (bytes, bytearray, memoryview)):
            raw = bytes(a)
            if len(raw) % 4:
                raise MsmError(_lib.MSM_ERR_ARG, f"{what}: {len(raw)} bytes are no array of 32-bit words")
            return (C.c_uint32 * max(len(raw) // 4, 1)).from_buffer_copy(raw or b"\0\0\0\0"), len(raw) // 4
        vals = [int(v) for v in (a.tolist() if hasattr(a, "tolist") else a)]
        if any(v < 0 or v >> 32 for v in vals):
            raise MsmError(_lib.MSM_ERR_ARG, f"{what}: an entry does not fit 32 bits")
        return (C.c_uint32 * max(len(vals), 1))(*vals), len(vals)

    def matrix_create(self, rows, cols: Optional[int] = None, row_ptr=None, col=None, val=None, nnz: Optional[int] = None,
                      on_device: bool = False, transpose: bool = False) -> int:
        """A resident sparse matrix in CSR (msm_matrix_create); returns its id.  rows may be a CsrMatrix (matrix_from_triplets)
        in place of the five arguments.  Host input: row_ptr and col are sequences of ints, numpy arrays or little-endian bytes,
        val is nnz x 32 bytes, a sequence of ints below 2^256, or None (every coefficient is 1).  on_device: row_ptr, col and val
        are device addresses (val 0 or None: all ones) and nnz is given.  transpose (host input only): the handle holds the
        transposed matrix, cols x rows.  The context copies everything: the arrays are free again when this returns."""
        if isinstance(rows, CsrMatrix):
            m = rows
            rows, cols, row_ptr, col, val = m.rows, m.cols, m.row_ptr, m.col, m.val
        flags = _lib.MATRIX_TRANSPOSE if transpose else 0
        out = C.c_int32(-1)
        if on_device:
            if nnz is None:
                raise MsmError(_lib.MSM_ERR_ARG, "matrix_create: device input needs nnz")
            rc = self._lib.msm_matrix_create(self._h, rows, cols, nnz, C.c_void_p(row_ptr), C.c_void_p(col), C.c_void_p(val or 0), 1,
                                             flags, C.byref(out))
        else:
            rp, n_rp = self._u32_buf(row_ptr, "row_ptr")
            cb, n_col = self._u32_buf(col, "col")
            if n_rp != rows + 1:
                raise MsmError(_lib.MSM_ERR_ARG, f"matrix_create: row_ptr holds {n_rp} entries for {rows} rows")
            nnz = n_col if nnz is None else nnz
            vb = None
            if val is not None:
                raw = bytes(val) if isinstance(val, (bytes, bytearray, memoryview)) else b"".join(_scalar32(v, "a value") for v in val)
                if len(raw) != 32 * nnz or n_col != nnz:
                    raise MsmError(_lib.MSM_ERR_ARG, f"matrix_create: {n_col} column indices and {len(raw)} value bytes for nnz = {nnz}")
                vb = (C.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
            elif n_col != nnz:
                raise MsmError(_lib.MSM_ERR_ARG, f"matrix_create: {n_col} column indices for nnz = {nnz}")
            rc = self._lib.msm_matrix_create(self._h, rows, cols, nnz, rp, cb, vb, 0, flags, C.byref(out))
        self._check(rc)
        return int(out.value)

    def matrix_destroy(self, matrix_id: int) -> None:
        self._check(self._lib.msm_matrix_destroy(self._h, matrix_id))

    def matrix_info(self, matrix_id: int) -> Dict[str, int]:
        """{"rows", "cols", "nnz", "bytes"} of a matrix as it is held (msm_matrix_info): bytes = the device memory it takes."""
        r, c, z, b = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.msm_matrix_info(self._h, matrix_id, C.byref(r), C.byref(c), C.byref(z), C.byref(b)))
        return {"rows": int(r.value), "cols": int(c.value), "nnz": int(z.value), "bytes": int(b.value)}

    def scalars_matvec(self, matrix_id: int, dst: int, x: int, alpha=None, accumulate: bool = False) -> None:
        """dst = alpha M x mod q, plus the old dst with accumulate (msm_scalars_matvec).  dst: rows scalars, x: cols scalars, device
        addresses aligned to 16 bytes and disjoint; alpha: int or 32 bytes < q, None = 1."""
        abuf = None if alpha is None else self._scalar_buf(alpha, "alpha")
        self._check(self._lib.msm_scalars_matvec(self._h, matrix_id, C.c_void_p(dst), C.c_void_p(x), abuf,
                                                 _lib.MATVEC_ACCUMULATE if accumulate else 0))

    def fold_scalars(self, dev_ptr: int, n: int, lo_scalar, hi_scalar) -> int:
        """The in-place fold of the n scalars at dev_ptr: v[i] <- lo_scalar * v[i] + hi_scalar * v[i + n/2], i < n/2 (n even); the
        upper half stays as it was.  The scalar fold of an inner-product argument beside fold_points.  Returns n/2."""
        if n < 0 or n % 2:
            raise MsmError(_lib.MSM_ERR_ARG, f"fold_scalars: {n} scalars, not an even number")
        h = n // 2
        self.scalars_lincomb(dev_ptr, lo_scalar, dev_ptr, hi_scalar, dev_ptr + 32 * h, h)
        return h

    # -- window tables (msm_precompute, include/msm_hip.h) ------------------------------------
    def precompute(self, n: Optional[int] = None, c: Optional[int] = None, no_glv: bool = False, point_lo: int = 0) -> Tuple[int, int, int]:
        """Builds the window tables of the current point set -- of its points [point_lo, point_lo + n): the share of one rank of a
        points-split run -- for the plan msm_run(n, c) would use (no-op if present or if they do not fit the limit).
        Returns tables_info()."""
        opts = MsmOpts(c=c or 0, no_glv=int(no_glv), point_lo=point_lo)
        self._check(self._lib.msm_precompute(self._h, self.n_points if n is None else n, C.byref(opts)))
        return self.tables_info()

    def tables_info(self) -> Tuple[int, int, int]:
        """(window bits c, windows K of the plan they serve, bytes held) of the current point set's window tables; (0, 0, 0):
        none.  The set holds K tables where a run on them is one window group, ceil(K / 2) shared ones where it is two."""
        c, k, b = C.c_int32(), C.c_int32(), C.c_uint64()
        self._check(self._lib.msm_tables_info(self._h, C.byref(c), C.byref(k), C.byref(b)))
        return c.value, k.value, b.value

    def tables_range(self) -> Tuple[int, int]:
        """(first point, number of points) the current point set's window tables cover; (0, 0): none."""
        lo, n = C.c_uint64(), C.c_uint64()
        self._check(self._lib.msm_tables_range(self._h, C.byref(lo), C.byref(n)))
        return lo.value, n.value

    def set_tables_limit(self, nbytes: int) -> None:
        self._check(self._lib.msm_set_tables_limit(self._h, nbytes))

    def reserve(self, n: int, c: Optional[int] = None) -> None:
        """Everything a later run_device(n, c) would allocate or build, now (msm_reserve)."""
        opts = MsmOpts(c=c or 0)
        self._check(self._lib.msm_reserve(self._h, n, C.byref(opts)))

    def window_sums(self, scalars: Union[BytesLike, int], n: int, k_lo: int, k_hi: int, c: Optional[int] = None,
                    on_device: bool = False, point_lo: int = 0, by_window: bool = False,
                    bucket_shard: Tuple[int, int] = (0, 0), merged: bool = False) -> Tuple[bytes, Dict]:
        """Partition sums P_k, k in [k_lo, k_hi), over the resident points [point_lo, point_lo + n) (scalar i belongs to
        point point_lo + i): (k_hi - k_lo) x 144 bytes (X, Y, Z).  merged (msm_opts.merged_sums): the caller only combines the
        sums, so they may come back merged -- the first slot carries sum_k 2^(c (k - k_lo)) P_k, the others the identity -- and
        the call may run on window tables (of the whole set, or of exactly this range of the points).  With c=None such a call
        runs under plan(n, merged=True, point_lo=point_lo) from the first time on: take k_hi and the window for the combine from
        there; info["c"], info["K"] repeat it on every call, info["tables"] says whether the tables were there."""
        if k_hi <= k_lo or k_lo < 0:   # (0, 0) would mean "all windows" to the C side and overrun the 144-byte buffer below
            raise MsmError(_lib.MSM_ERR_ARG, f"empty or negative window range [{k_lo}, {k_hi})")
        # bucket_shard = (g, G): only the buckets [L g / G, L (g + 1) / G) of every window (msm_opts.bucket_shard)
        opts = MsmOpts(c=c or 0, k_lo=k_lo, k_hi=k_hi, point_lo=point_lo, by_window=int(by_window),
                       bucket_shard=bucket_shard[0], bucket_shards=bucket_shard[1], merged_sums=int(merged))
        res = MsmResult()
        out = (C.c_uint8 * (144 * max(k_hi - k_lo, 1)))()
        if on_device:
            ptr = C.c_void_p(int(scalars))
        elif isinstance(scalars, C.Array):
            ptr = scalars   # handed over as it is (no copy of a 2 GB buffer)
        else:
            ptr = (C.c_uint8 * max(32 * n, 1)).from_buffer_copy(bytes(scalars) or b"\0")
        self._check(self._lib.msm_window_sums(self._h, ptr, n, int(on_device), C.byref(opts), out, C.byref(res)))
        return bytes(out)[: 144 * (k_hi - k_lo)], _result_to_dict(res)

    def combine(self, partials: BytesLike, K: int, c: int) -> AffineResult:
        buf = (C.c_uint8 * len(partials)).from_buffer_copy(bytes(partials))
        res = MsmResult()
        self._check(self._lib.msm_combine(self._h, buf, K, c, C.byref(res)))
        nb = self.coord_bytes
        return AffineResult(int.from_bytes(bytes(res.x)[:nb], "little"), int.from_bytes(bytes(res.y)[:nb], "little"), bool(res.is_infinity))

    # -- fine-grained operators (GPU test kernels) -------------------------------------------
    def test_fp(self, op: int, a: BytesLike, b: Optional[BytesLike] = None) -> bytes:
        nb = self.coord_bytes
        n = len(a) // nb
        b = a if b is None else b
        ba = (C.c_uint8 * len(a)).from_buffer_copy(bytes(a))
        bb = (C.c_uint8 * len(b)).from_buffer_copy(bytes(b))
        out = (C.c_uint8 * len(a))()
        self._check(self._lib.msm_test_fp(self._h, op, ba, bb, out, n))
        return bytes(out)

    def test_glv(self, scalars: BytesLike) -> List[Tuple[int, int, bool, bool]]:
        n = len(scalars) // 32
        bs = (C.c_uint8 * len(scalars)).from_buffer_copy(bytes(scalars))
        out = (C.c_uint8 * (40 * n))()
        self._check(self._lib.msm_test_glv(self._h, bs, out, n))
        raw = bytes(out)
        res = []
        for i in range(n):
            r = raw[40 * i : 40 * i + 40]
            res.append((int.from_bytes(r[:16], "little"), int.from_bytes(r[16:32], "little"),
                        bool(int.from_bytes(r[32:36], "little")), bool(int.from_bytes(r[36:40], "little"))))
        return res

    def test_batch_inverse(self, xs: BytesLike, per_lane: int = 7) -> bytes:
        n = len(xs) // self.coord_bytes
        bx = (C.c_uint8 * len(xs)).from_buffer_copy(bytes(xs))
        out = (C.c_uint8 * len(xs))()
        self._check(self._lib.msm_test_batch_inverse(self._h, bx, out, n, per_lane))
        return bytes(out)

    def test_fp_raw(self, op: int, a_limbs: Sequence[Sequence[int]], b_limbs: Sequence[Sequence[int]]) -> List[List[int]]:
        """fe_mul / fe_sqr on raw 30-bit-limb operands (lists of NL ints per element); returns the raw result limbs."""
        nl = 9 if self.curve in _lib.CURVES_32_BYTE else 13   # limbs are sized per field
        n = len(a_limbs)
        A = (C.c_uint32 * (nl * n))(*[w for e in a_limbs for w in e])
        B = (C.c_uint32 * (nl * n))(*[w for e in b_limbs for w in e])
        out = (C.c_uint32 * (nl * n))()
        self._check(self._lib.msm_test_fp_raw(self._h, op, A, B, out, n))
        return [[int(out[i * nl + j]) for j in range(nl)] for i in range(n)]

    def test_curve_op(self, op: int, p: BytesLike, q: BytesLike) -> bytes:
        """Projective (X || Y || Z, one coordinate width each) or extended Edwards (X || Y || Z || T, 32 B each) operator; see
        msm_hip.h."""
        bp = (C.c_uint8 * len(p)).from_buffer_copy(bytes(p))
        bq = (C.c_uint8 * len(q)).from_buffer_copy(bytes(q))
        out = (C.c_uint8 * len(p))()
        nb = 128 if self.curve == _lib.CURVE_ED_ON_BLS12_377 else 3 * self.coord_bytes
        self._check(self._lib.msm_test_curve_op(self._h, op, bp, bq, out, len(p) // nb))
        return bytes(out)

    def test_batch_add_mode(self, g: BytesLike, h: BytesLike, mode: int, steps: int) -> bytes:
        n = len(g) // (2 * self.coord_bytes)
        bg = (C.c_uint8 * len(g)).from_buffer_copy(bytes(g))
        bh = (C.c_uint8 * len(h)).from_buffer_copy(bytes(h))
        out = (C.c_uint8 * len(g))()
        self._check(self._lib.msm_test_batch_add_mode(self._h, bg, bh, out, n, mode, steps))
        return bytes(out)

    def test_bucket_reduce(self, buckets: BytesLike, K: int, L: int, mode: int = 0, c0: int = 2) -> Tuple[bytes, float]:
        """P_k = sum_l l B_(k,l) for K windows of L buckets (x || y, 48-byte LE each, (0, 0) = empty): K x 144 bytes (X, Y, Z)
        and the device time in ms.  mode 0: the projective reduction of the MSM; mode 1: the reference's all-affine
        reduction (reduceBucketsAffine) out of in-place batched additions, chunks of 2^c0 buckets."""
        if len(buckets) != 2 * self.coord_bytes * K * L:
            raise MsmError(_lib.MSM_ERR_ARG, f"expected {2 * self.coord_bytes * K * L} bytes of buckets, got {len(buckets)}")
        buf = (C.c_uint8 * len(buckets)).from_buffer_copy(bytes(buckets))
        out = (C.c_uint8 * (144 * K))()
        ms = C.c_float(0)
        self._check(self._lib.msm_test_bucket_reduce(self._h, buf, K, L, mode, c0, out, C.byref(ms)))
        return bytes(out), float(ms.value)

    def test_bucket_sums(self, pool: BytesLike, off, elems, K: int, L: int, merged: bool = False, stride: int = 0, tc: int = 0,
                         want_perm: bool = False):
        """The bucket finish and the bucket reduction of the pipeline on crafted buckets (msm_test_bucket_sums, msm_hip.h): `pool`
        = affine wire points, bucket l of window k = the pool points elems[off[k L + l - 1] : off[k L + l]] (uint32 arrays).
        Returns K x 144 bytes (X || Y || Z per slot); with want_perm also the K L bucket indices in the order the finish took them."""
        import numpy as np

        off = np.ascontiguousarray(off, dtype=np.uint32)
        elems = np.ascontiguousarray(elems, dtype=np.uint32)
        pb = 2 * self.coord_bytes
        if len(pool) == 0 or len(pool) % pb or len(off) != K * L + 1 or len(elems) != int(off[-1]):
            raise MsmError(_lib.MSM_ERR_ARG, f"expected whole {pb}-byte pool points, {K * L + 1} offsets and off[-1] elements")
        buf = (C.c_uint8 * len(pool)).from_buffer_copy(bytes(pool))
        out = (C.c_uint8 * (144 * K))()
        perm = np.empty(K * L, dtype=np.uint32) if want_perm else None
        self._check(self._lib.msm_test_bucket_sums(self._h, buf, len(pool) // pb, off.ctypes.data, elems.ctypes.data if len(elems) else None,
                                                   K, L, int(bool(merged)), stride, tc, out, perm.ctypes.data if want_perm else None))
        return (bytes(out), perm) if want_perm else bytes(out)

    TREE_MODES = ("gather", "regular", "search")

    def test_tree_sums(self, pool: BytesLike, off, elems, K: int, L: int, c: int, logG: int, flags=None, reported_max: int = 0,
                       tail_tables: int = 0, want_cursor: bool = True) -> dict:
        """The scans behind the sort, the round plan and every round of the accumulation tree on crafted buckets, then the bucket
        reduction (msm_test_tree_sums, msm_hip.h).  pool, off, elems, K, L as test_bucket_sums; flags: one uint8 per element
        (bit 0 negate, bit 1 the beta x line) or None; c picks the threshold class, logG the padding granule; reported_max
        stands in for the largest bucket (0: the device finds it).  tail_tables: how many tail_off tables to bring back.
        Returns {"sums": K x 144 bytes, "RT", "r_stop", "total_slots", "max_bucket", "rounds", "n_pairs", "cursor": uint32
        [K L + 1] or None, "tail_off": uint32 [min(RT + 1, tail_tables), K L + 1], "log": [(mode name, n_out, steps), ...]}."""
        import numpy as np

        off = np.ascontiguousarray(off, dtype=np.uint32)
        elems = np.ascontiguousarray(elems, dtype=np.uint32)
        pb = 2 * self.coord_bytes
        if len(pool) == 0 or len(pool) % pb or len(off) != K * L + 1 or len(elems) != int(off[-1]):
            raise MsmError(_lib.MSM_ERR_ARG, f"expected whole {pb}-byte pool points, {K * L + 1} offsets and off[-1] elements")
        if flags is not None:
            flags = np.ascontiguousarray(flags, dtype=np.uint8)
            if len(flags) != len(elems):
                raise MsmError(_lib.MSM_ERR_ARG, "expected one flag byte per element")
        buf = (C.c_uint8 * len(pool)).from_buffer_copy(bytes(pool))
        out = (C.c_uint8 * (144 * K))()
        plan = np.zeros(8, dtype=np.uint64)
        cursor = np.zeros(K * L + 1, dtype=np.uint32) if want_cursor else None
        tail = np.zeros((max(tail_tables, 0), K * L + 1), dtype=np.uint32)
        LOG_CAP = 48   # logG <= 10 regular and RT <= 32 tail rounds
        log = np.zeros((LOG_CAP, 3), dtype=np.uint64)
        self._check(self._lib.msm_test_tree_sums(
            self._h, buf, len(pool) // pb, off.ctypes.data, elems.ctypes.data if len(elems) else None,
            flags.ctypes.data if flags is not None and len(flags) else None, K, L, c, logG, reported_max, out, plan.ctypes.data,
            cursor.ctypes.data if want_cursor else None, tail.ctypes.data if tail_tables > 0 else None, max(tail_tables, 0),
            log.ctypes.data, LOG_CAP))
        RT, r_stop, total_slots, max_bucket, rounds, n_pairs, n_log = (int(v) for v in plan[:7])
        return {"sums": bytes(out), "RT": RT, "r_stop": r_stop, "total_slots": total_slots, "max_bucket": max_bucket, "rounds": rounds,
                "n_pairs": n_pairs, "cursor": cursor, "tail_off": tail[:min(RT + 1, max(tail_tables, 0))],
                "log": [(self.TREE_MODES[int(m)], int(n), int(s)) for m, n, s in log[:min(n_log, LOG_CAP)]]}

    def test_set_chunk_rows_log(self, log2_rows: int = 0) -> None:
        """Round 1 of big windows takes the pair form above 2^log2_rows table rows (msm_test_set_chunk_rows_log, msm_hip.h);
        0 restores the default of 23."""
        self._check(self._lib.msm_test_set_chunk_rows_log(self._h, log2_rows))

    @staticmethod
    def test_live_buffers() -> Tuple[int, int]:
        """(count, bytes) of the device buffers the library holds in this process, over all contexts, the bytes as allocated
        (msm_test_live_buffers, msm_hip.h).  Needs no context and stays readable after close()."""
        count, nbytes = C.c_uint64(), C.c_uint64()
        rc = _lib.load().msm_test_live_buffers(C.byref(count), C.byref(nbytes))
        if rc != _lib.MSM_OK:
            raise MsmError(rc, "msm_test_live_buffers failed")
        return int(count.value), int(nbytes.value)

    def test_last_sort_paths(self) -> List[str]:
        """The sort path of every window group of the last call, in schedule order: "one_level", "radix", "slots" or "pairs"
        (msm_test_last_sort_paths, msm_hip.h)."""
        count = self._lib.msm_test_last_sort_paths(self._h, None, 0)
        if count < 0:
            raise MsmError(_lib.MSM_ERR_ARG, "msm_test_last_sort_paths: not on a device-list context")
        out = (C.c_int32 * max(count, 1))()
        self._lib.msm_test_last_sort_paths(self._h, out, count)
        if any(not 0 <= v < len(_lib.SORT_PATH_NAMES) for v in out[:count]):
            raise MsmError(_lib.MSM_ERR_INTERNAL, f"msm_test_last_sort_paths: unknown sort path in {list(out[:count])}")
        return [_lib.SORT_PATH_NAMES[v] for v in out[:count]]

    def test_digits(self, scalars, n: Optional[int] = None, first: int = 0, width: int = 0, bits: int = 0, signed: bool = False,
                    c: int = 0, no_glv: bool = False, strict: bool = False, bucket_shard: int = 0, bucket_shards: int = 0,
                    k_lo: int = 0, k_hi: int = 0) -> dict:
        """The window digits of a call's scalars from the digit kernel alone (msm_test_digits, msm_hip.h).  scalars: one uint8
        array of whole scalars (32 bytes each, or `width` bytes of the narrow format (width, bits, signed)), or a list of B >= 2
        such arrays for the fused batch.  The call's scalars are the elements [first, first + n) of the array (n: the rest).
        Returns {"rc": what the real call makes of the kernel's error word, "c", "K", "fold", "words": uint32 array of shape
        (windows, 2 n) -- Ed-on-BLS12-377: (windows, n); a batch: (B, K, ...)}; raises MsmError where the plan is refused."""
        import numpy as np

        batch = isinstance(scalars, (list, tuple))
        wb = width or 32
        arrs = [np.ascontiguousarray(np.frombuffer(bytes(a), dtype=np.uint8) if isinstance(a, (bytes, bytearray)) else a, dtype=np.uint8).reshape(-1)
                for a in (scalars if batch else [scalars])]
        if not arrs or any(len(a) != len(arrs[0]) or len(a) % wb for a in arrs):
            raise MsmError(_lib.MSM_ERR_ARG, f"expected arrays of whole {wb}-byte scalars, all of one length")
        n_array = len(arrs[0]) // wb
        if n is None:
            n = n_array - first
        if n <= 0 or first < 0 or first + n > n_array:
            raise MsmError(_lib.MSM_ERR_ARG, f"scalars [{first}, {first} + {n}) of an array of {n_array}")
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        opts = MsmOpts(c=c or 0, no_glv=int(no_glv), strict=int(strict), bucket_shard=bucket_shard, bucket_shards=bucket_shards)
        per = 1 if self.curve == _lib.CURVE_ED_ON_BLS12_377 else 2
        cc, K, fold, frc = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        args = (self._h, ptrs, len(arrs), n, n_array, first, width, bits, int(bool(signed)), C.byref(opts), k_lo, k_hi)
        # the plan first (no output buffer: nothing runs), then a buffer of exactly its rows
        self._check(self._lib.msm_test_digits(*args, None, C.byref(cc), C.byref(K), C.byref(fold), None))
        rows = k_hi - k_lo if (k_lo or k_hi) else K.value
        out = np.empty((len(arrs), rows, per * n) if batch else (rows, per * n), dtype=np.uint32)
        self._check(self._lib.msm_test_digits(*args, out.ctypes.data, C.byref(cc), C.byref(K), C.byref(fold), C.byref(frc)))
        return {"rc": frc.value, "c": cc.value, "K": K.value, "fold": bool(fold.value), "words": out}

    def test_batch_add(self, g: BytesLike, h: BytesLike) -> bytes:
        n = len(g) // (2 * self.coord_bytes)
        bg = (C.c_uint8 * len(g)).from_buffer_copy(bytes(g))
        bh = (C.c_uint8 * len(h)).from_buffer_copy(bytes(h))
        out = (C.c_uint8 * len(g))()
        self._check(self._lib.msm_test_batch_add(self._h, bg, bh, out, n))
        return bytes(out)


# ---------------------------------------------------------------------------------------------
# reference-shaped facade
# ---------------------------------------------------------------------------------------------


class PointPtr:
    """Handle standing in for the reference's `pointPtr` (byte offset of an affine point array): one resident point set
    of the context, its own allocation like every pointer of the reference; freed when the handle goes away."""

    def __init__(self, ctx: Optional["MsmContext"] = None, size: int = 0, n: int = 0, set_id: int = 0):
        self._ctx, self.size, self.n, self.set_id = ctx, size, n, set_id

    def close(self) -> None:
        ctx, self._ctx = self._ctx, None
        if ctx is not None and self.set_id > 0 and getattr(ctx, "_h", None):
            ctx.pointset_destroy(self.set_id)

    def __iter__(self):
        """`[pointPtr] = Parallel.randomPointsFast(N)`: the reference returns one pointer per point and its callers keep the first
        (scripts/msm-weierstrass.ts:18); a handle here stands for the whole array and unpacks to itself."""
        yield self

    def __enter__(self) -> "PointPtr":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScalarPtr:
    """Handle standing in for `scalarPtr`: host bytes (`scalarsFromBytes`) or a device buffer of its own
    (`randomScalars`); the device buffer is freed when the handle goes away."""

    def __init__(self, ctx: Optional["MsmContext"] = None, size: int = 0, data: bytes = b"", dev_ptr: int = 0, n: int = 0):
        self._ctx, self.size, self.data, self.dev_ptr, self.n = ctx, size, data, dev_ptr, n

    def close(self) -> None:
        ctx, self._ctx = self._ctx, None
        if ctx is not None and self.dev_ptr and getattr(ctx, "_h", None):
            ctx.device_free(self.dev_ptr)
        self.dev_ptr = 0

    def __iter__(self):
        """`[scalarPtr] = Parallel.randomScalars(N)` (scripts/msm-weierstrass.ts:21,29): unpacks to itself."""
        yield self

    def __enter__(self) -> "ScalarPtr":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Parallel:
    """`Curve.Parallel` (src/parallel.ts:135-145 Weierstrass, :251-259 twisted Edwards)."""

    def __init__(self, ctx: MsmContext, params):
        self._ctx = ctx
        self._params = params
        # wire bytes per coordinate = the reference's packed field size (src/wasm/field-helpers.ts:211-301) = the C ABI's
        self._wire_bytes = (params.modulus.bit_length() + 7) // 8 if hasattr(params, "modulus") else ctx.coord_bytes

    def getPointer(self, size: int) -> PointPtr:
        return PointPtr(self._ctx, size=size, set_id=self._ctx.pointset_create())

    def getScalarPointer(self, size: int) -> ScalarPtr:
        return ScalarPtr(self._ctx, size=size)

    def pointsFromBytes(self, pointPtr: PointPtr, pointInput: BytesLike, n: int, compressed: bool = False,
                        validate: Optional[str] = None) -> None:
        """src/parallel.ts:97-116 (96 B/point) / :215-229 (64 B/point): x || y little-endian -> resident device points.
        compressed: the compressed encoding of the curve instead (MsmContext.load_points); validate: None (default, as the
        reference), "curve" or "subgroup"."""
        if compressed or validate is not None:
            self._ctx.pointset_select(pointPtr.set_id)
            pointPtr.n = 0
            step = self._ctx.coord_bytes * (1 if compressed else 2)
            self._ctx.load_points(bytes(pointInput)[: step * n], compressed=compressed, validate=validate)
            pointPtr.n = n
            return
        wb, cb = self._wire_bytes, self._ctx.coord_bytes
        buf = bytes(pointInput)[: 2 * wb * n]
        if wb != cb:   # zero-pad every coordinate to the ABI width
            import numpy as np

            padded = np.zeros((2 * n, cb), dtype=np.uint8)
            padded[:, :wb] = np.frombuffer(buf, dtype=np.uint8).reshape(2 * n, wb)
            buf = padded.tobytes()
        self._ctx.pointset_select(pointPtr.set_id)
        self._ctx.set_points(buf)
        pointPtr.n = n

    def scalarsFromBytes(self, scalarPtr: ScalarPtr, scalarInput: BytesLike, n: int) -> None:
        """src/parallel.ts:119-133: n scalars of 32 bytes little-endian."""
        scalarPtr.data = bytes(scalarInput)[: 32 * n]
        scalarPtr.dev_ptr = 0
        scalarPtr.n = n

    def randomPointsFast(self, n: int, seed: int = 1) -> PointPtr:
        """src/curve-random.ts:14-92 (generated on the GPU; the seed is explicit, the reference is unseeded)."""
        ptr = self.getPointer(2 * self._wire_bytes * n)
        self._ctx.generate_points(n, seed)
        ptr.n = n
        return ptr

    def randomScalars(self, n: int, seed: int = 1) -> ScalarPtr:
        """src/curve-random.ts:151-194."""
        dev = self._ctx.device_alloc(32 * max(n, 1))   # the handle's own buffer: two handles never alias
        self._ctx.generate_scalars(n, seed, into=dev)
        return ScalarPtr(self._ctx, size=32 * n, dev_ptr=dev, n=n)

    def msm(self, scalarPtr: ScalarPtr, pointPtr: PointPtr, N: int, verboseTiming: bool = False,
            options: Optional[Dict] = None) -> Dict:
        """`msm` (src/msm-batched-affine.ts:69-340): returns {"result": AffineResult, "log": [...]}.
        options: {"c": window bits, "useSafeAdditions": bool}."""
        options = options or {}
        self._ctx.pointset_select(pointPtr.set_id)
        if N > pointPtr.n or N > self._ctx.n_points:
            raise MsmError(_lib.MSM_ERR_NO_POINTS, f"{N} scalars but {min(pointPtr.n, self._ctx.n_points)} points behind this pointer")
        if N > scalarPtr.n:
            raise MsmError(_lib.MSM_ERR_ARG, f"{N} scalars requested but the scalar pointer holds {scalarPtr.n}")
        unsafe = not options.get("useSafeAdditions", True)
        no_glv = bool(options.get("noGlv", False))
        if scalarPtr.dev_ptr:
            res, info = self._ctx.run_device(scalarPtr.dev_ptr, N, options.get("c"), unsafe, no_glv=no_glv)
        else:
            res, info = self._ctx.run(scalarPtr.data[: 32 * N], options.get("c"), unsafe, no_glv=no_glv)
        log: List = []
        if verboseTiming:
            # the reference's shape (createLog, src/msm-common.ts:176-214, filled at src/msm-batched-affine.ts:79-338): the
            # parameters first, one "label... x.xms" line per phase under the reference's labels, "msm total" last
            t = info["phase_ms"]
            log.append([{"n": (N - 1).bit_length() if N > 1 else 0, "K": info["K"], "c": info["c"]}])
            for label, key in (("scalars to device", "upload"), ("slice scalars & count buckets", "digits"), ("sort points", "sort"),
                               ("bucket accumulation (first round)", "accumulate_round1"), ("bucket accumulation", "accumulate"),
                               ("bucket reduction (local)", "reduce"), ("final sum", "final"), ("msm total", "total")):
                log.append([f"{label}... {t[key]:.1f}ms"])
        return {"result": res, "log": log, "info": info}

    def msmBatch(self, scalarPtrs: Sequence[ScalarPtr], pointPtr: PointPtr, N: int, verboseTiming: bool = False,
                 options: Optional[Dict] = None) -> List[Dict]:
        """Many MSMs over one point set in one call (msm_run_batch): one dict per scalar pointer, shaped like msm's, whose
        "result" equals msm(scalarPtrs[b], pointPtr, N)["result"].  The scalar pointers are all on the device or all on the host."""
        options = options or {}
        self._ctx.pointset_select(pointPtr.set_id)
        if N > pointPtr.n or N > self._ctx.n_points:
            raise MsmError(_lib.MSM_ERR_NO_POINTS, f"{N} scalars but {min(pointPtr.n, self._ctx.n_points)} points behind this pointer")
        for sp in scalarPtrs:
            if N > sp.n:
                raise MsmError(_lib.MSM_ERR_ARG, f"{N} scalars requested but a scalar pointer holds {sp.n}")
        on_dev = [bool(sp.dev_ptr) for sp in scalarPtrs]
        if any(on_dev) and not all(on_dev):
            raise MsmError(_lib.MSM_ERR_ARG, "msmBatch: the scalar pointers must all be on the device or all on the host")
        unsafe = not options.get("useSafeAdditions", True)
        no_glv = bool(options.get("noGlv", False))
        if scalarPtrs and all(on_dev):
            out = self._ctx.run_batch_device([sp.dev_ptr for sp in scalarPtrs], N, options.get("c"), unsafe, no_glv=no_glv)
        else:
            out = self._ctx.run_batch([sp.data[: 32 * N] for sp in scalarPtrs], options.get("c"), unsafe, no_glv=no_glv)
        dicts = []
        for res, info in out:
            log: List = []
            if verboseTiming:
                t = info["phase_ms"]
                log.append([{"n": (N - 1).bit_length() if N > 1 else 0, "K": info["K"], "c": info["c"], "batch": len(scalarPtrs)}])
                for label, key in (("scalars to device", "upload"), ("slice scalars & count buckets", "digits"), ("sort points", "sort"),
                                   ("bucket accumulation (first round)", "accumulate_round1"), ("bucket accumulation", "accumulate"),
                                   ("bucket reduction (local)", "reduce"), ("final sum", "final"), ("msm total", "total")):
                    log.append([f"{label}... {t[key]:.1f}ms"])
            dicts.append({"result": res, "log": log, "info": info})
        return dicts

    def msmNarrow(self, scalars, pointPtr: PointPtr, N: int, options: Optional[Dict] = None) -> Dict:
        """MSM over narrow scalars (msm_run_narrow; the reference has no counterpart): `scalars` is a numpy array of dtype
        uint8/16/32/64 or int8/16/32/64, or bytes with options["width"]; options: {"c", "bits", "signed", "width"}.
        Returns msm's shape, {"result", "log", "info"}; "result" equals msm over the same values as 32-byte scalars."""
        options = options or {}
        self._ctx.pointset_select(pointPtr.set_id)
        if N > pointPtr.n or N > self._ctx.n_points:
            raise MsmError(_lib.MSM_ERR_NO_POINTS, f"{N} scalars but {min(pointPtr.n, self._ctx.n_points)} points behind this pointer")
        if hasattr(scalars, "dtype"):
            if N > scalars.size:
                raise MsmError(_lib.MSM_ERR_ARG, f"{N} scalars requested but the array holds {scalars.size}")
            scalars = scalars.ravel()[:N]
        else:
            w = options.get("width") or 0
            if w <= 0 or N * w > len(scalars):
                raise MsmError(_lib.MSM_ERR_ARG, f"{N} scalars of width {w} requested but the buffer holds {len(scalars)} bytes")
            scalars = bytes(scalars)[: N * w]
        res, info = self._ctx.run_narrow(scalars, options.get("bits"), options.get("signed"), options.get("c"),
                                         width=options.get("width"))
        return {"result": res, "log": [], "info": info}

    def msmIndexed(self, scalars, indices, pointPtr: PointPtr, options: Optional[Dict] = None) -> Dict:
        """Indexed (sparse) MSM (msm_run_indexed; the reference has no counterpart): sum_j scalars[j] * P[indices[j]] over the
        points behind pointPtr.  scalars: bytes of m x 32 or a uint8 array (m, 32); indices: m integers, any order, repeats
        allowed; options: {"c", "noGlv"}.  Returns msm's shape; "result" equals msm over the dense equivalent."""
        options = options or {}
        self._ctx.pointset_select(pointPtr.set_id)
        res, info = self._ctx.msm_indexed(scalars, indices, c=options.get("c"), no_glv=bool(options.get("noGlv", False)))
        return {"result": res, "log": [], "info": info}

    def msmIndexedNarrow(self, scalars, indices, pointPtr: PointPtr, options: Optional[Dict] = None) -> Dict:
        """msmIndexed over narrow scalars (msm_run_indexed_narrow): scalars and options {"c", "bits", "signed", "width"} as for
        msmNarrow."""
        options = options or {}
        self._ctx.pointset_select(pointPtr.set_id)
        res, info = self._ctx.msm_indexed_narrow(scalars, indices, bits=options.get("bits"), signed=options.get("signed"),
                                                 c=options.get("c"), width=options.get("width"))
        return {"result": res, "log": [], "info": info}

    def pointsLincomb(self, dstPtr: PointPtr, a, ptrA: PointPtr, b=None, ptrB: Optional[PointPtr] = None,
                      options: Optional[Dict] = None) -> PointPtr:
        """dstPtr[i] = a * ptrA[aLo + i] + b * ptrB[bLo + i], i < count (msm_points_lincomb; the reference has no counterpart).
        a, b: ints or 32 bytes, < q; b None: one term.  options: {"aLo", "bLo", "count"} (count: default all of ptrA from aLo on).
        dstPtr may be ptrA or ptrB; it then holds `count` points.  Returns dstPtr."""
        options = options or {}
        if (b is None) != (ptrB is None):
            raise MsmError(_lib.MSM_ERR_ARG, "pointsLincomb: b and ptrB come together")
        a_lo, b_lo = int(options.get("aLo", 0)), int(options.get("bLo", 0))
        count = options.get("count")
        count = self._ctx.points_lincomb(a, b, src_a=ptrA.set_id, a_lo=a_lo, src_b=None if ptrB is None else ptrB.set_id, b_lo=b_lo,
                                         count=max(ptrA.n - a_lo, 0) if count is None else count, dst=dstPtr.set_id)
        dstPtr.n = count
        return dstPtr

    def foldPoints(self, pointPtr: PointPtr, a, b) -> PointPtr:
        """The in-place fold of the points behind pointPtr: P[i] <- a * P[i] + b * P[i + n/2]; the pointer then holds n/2 points
        (MsmContext.fold_points)."""
        self._ctx.pointset_select(pointPtr.set_id)
        pointPtr.n = self._ctx.fold_points(a, b)
        return pointPtr

    # -- scalar vectors on the device (msm_scalars_*; the reference has no counterpart) ------------
    def _scalar_dev(self, ptr: ScalarPtr, n: int, what: str, alloc: bool = False) -> int:
        """The device address behind a scalar pointer that holds at least n scalars; host bytes move to a buffer of the pointer's
        own first.  alloc: a destination, which gets a buffer of n scalars if it has none that large."""
        if alloc and (not ptr.dev_ptr or ptr.n < n):
            if ptr.dev_ptr:
                self._ctx.device_free(ptr.dev_ptr)
            ptr._ctx, ptr.dev_ptr, ptr.data = self._ctx, self._ctx.device_alloc(32 * max(n, 1)), b""
            ptr.n, ptr.size = n, 32 * n
        if not ptr.dev_ptr and ptr.data:
            dev = self._ctx.device_alloc(max(len(ptr.data), 32))
            self._ctx.device_upload(dev, ptr.data)
            ptr._ctx, ptr.dev_ptr, ptr.data = self._ctx, dev, b""
        if n > ptr.n or (n and not ptr.dev_ptr):
            raise MsmError(_lib.MSM_ERR_ARG, f"{what}: {n} scalars requested but the scalar pointer holds {ptr.n}")
        return ptr.dev_ptr

    def scalarsLincomb(self, dstPtr: ScalarPtr, x, ptrA: ScalarPtr, y=None, ptrB: Optional[ScalarPtr] = None,
                       options: Optional[Dict] = None) -> ScalarPtr:
        """dstPtr[i] = x * ptrA[aLo + i] + y * ptrB[bLo + i] mod q, i < count.  options: {"aLo", "bLo", "count"} (count: default
        all of ptrA from aLo on).  dstPtr may be ptrA or ptrB (with an offset of 0); it then holds at least `count` scalars."""
        options = options or {}
        if (y is None) != (ptrB is None):
            raise MsmError(_lib.MSM_ERR_ARG, "scalarsLincomb: y and ptrB come together")
        a_lo, b_lo = int(options.get("aLo", 0)), int(options.get("bLo", 0))
        count = options.get("count")
        count = max(ptrA.n - a_lo, 0) if count is None else int(count)
        a = self._scalar_dev(ptrA, a_lo + count, "scalarsLincomb")
        b = None if ptrB is None else self._scalar_dev(ptrB, b_lo + count, "scalarsLincomb")
        d = self._scalar_dev(dstPtr, count, "scalarsLincomb", alloc=True)
        self._ctx.scalars_lincomb(d, x, a + 32 * a_lo, y, None if b is None else b + 32 * b_lo, count)
        return dstPtr

    def scalarsMul(self, dstPtr: ScalarPtr, ptrA: ScalarPtr, ptrB: ScalarPtr, N: int) -> ScalarPtr:
        """dstPtr[i] = ptrA[i] * ptrB[i] mod q, i < N."""
        a, b = self._scalar_dev(ptrA, N, "scalarsMul"), self._scalar_dev(ptrB, N, "scalarsMul")
        self._ctx.scalars_mul(self._scalar_dev(dstPtr, N, "scalarsMul", alloc=True), a, b, N)
        return dstPtr

    def scalarsInner(self, ptrA: ScalarPtr, ptrB: ScalarPtr, N: int, options: Optional[Dict] = None) -> int:
        """sum_i ptrA[aLo + i] * ptrB[bLo + i] mod q, i < N, as an int.  options: {"aLo", "bLo"}."""
        options = options or {}
        a_lo, b_lo = int(options.get("aLo", 0)), int(options.get("bLo", 0))
        a, b = self._scalar_dev(ptrA, a_lo + N, "scalarsInner"), self._scalar_dev(ptrB, b_lo + N, "scalarsInner")
        return self._ctx.scalars_inner(a + 32 * a_lo, b + 32 * b_lo, N)

    def scalarsPowers(self, x, N: int, s=1) -> ScalarPtr:
        """A new scalar pointer holding (s, s x, s x^2, ..., s x^(N-1)) mod q."""
        ptr = ScalarPtr(self._ctx, size=32 * N)
        self._ctx.scalars_powers(self._scalar_dev(ptr, N, "scalarsPowers", alloc=True), x, N, s)
        return ptr

    def scalarsNtt(self, dstPtr: ScalarPtr, ptr: ScalarPtr, log2n: int, options: Optional[Dict] = None) -> ScalarPtr:
        """dstPtr = the transform of the `batch` vectors of 2^log2n scalars at the start of ptr (MsmContext.scalars_ntt).
        options: {"inverse", "omega", "shift", "batch"}.  dstPtr may be ptr."""
        options = options or {}
        batch = int(options.get("batch", 1))
        count = batch << log2n
        a = self._scalar_dev(ptr, count, "scalarsNtt")
        d = self._scalar_dev(dstPtr, count, "scalarsNtt", alloc=True)
        self._ctx.scalars_ntt(d, a, log2n, bool(options.get("inverse", False)), options.get("omega"), options.get("shift"), batch)
        return dstPtr

    def scalarsRootOfUnity(self, log2n: int) -> int:
        """The library's primitive 2^log2n-th root of unity mod q (MsmContext.scalars_root_of_unity)."""
        return self._ctx.scalars_root_of_unity(log2n)

    def scalarsScan(self, dstPtr: ScalarPtr, ptr: ScalarPtr, N: int, options: Optional[Dict] = None) -> int:
        """dstPtr = the running sum or product of the first N scalars of ptr (MsmContext.scalars_scan); returns the total.
        options: {"op": "sum" | "product", "exclusive", "init"}.  dstPtr may be ptr."""
        options = options or {}
        a = self._scalar_dev(ptr, N, "scalarsScan")
        d = self._scalar_dev(dstPtr, N, "scalarsScan", alloc=True)
        return self._ctx.scalars_scan(d, a, N, options.get("op", "sum"), bool(options.get("exclusive", False)), options.get("init"))

    def scalarsInverse(self, dstPtr: ScalarPtr, ptr: ScalarPtr, N: int) -> int:
        """dstPtr[i] = ptr[i]^-1 mod q, 0 where the residue is 0; returns how many of those there were
        (MsmContext.scalars_inverse).  dstPtr may be ptr."""
        a = self._scalar_dev(ptr, N, "scalarsInverse")
        return self._ctx.scalars_inverse(self._scalar_dev(dstPtr, N, "scalarsInverse", alloc=True), a, N)

    def scalarsDivLinear(self, dstPtr: ScalarPtr, ptr: ScalarPtr, N: int, z) -> int:
        """dstPtr = the quotient of the polynomial with the N coefficients of ptr by X - z, dstPtr[N-1] = 0; returns the
        remainder, its value at z (MsmContext.scalars_div_linear).  dstPtr may be ptr."""
        a = self._scalar_dev(ptr, N, "scalarsDivLinear")
        return self._ctx.scalars_div_linear(self._scalar_dev(dstPtr, N, "scalarsDivLinear", alloc=True), a, N, z)

    def scalarsSumcheckRound(self, ptrs: List[ScalarPtr], log2n: int, variable: int, options: Optional[Dict] = None) -> List[int]:
        """The round polynomial s(0 .. d) of a sumcheck over the tables of 2^log2n scalars at the start of each pointer
        (MsmContext.scalars_sumcheck_round).  options: {"shape": "prod" | "r1cs"}."""
        options = options or {}
        n = 1 << log2n
        devs = [self._scalar_dev(p, n, "scalarsSumcheckRound") for p in ptrs]
        return self._ctx.scalars_sumcheck_round(devs, log2n, variable, options.get("shape", "prod"))

    def scalarsBind(self, ptrs: List[ScalarPtr], log2n: int, variable: int, r, options: Optional[Dict] = None) -> List[ScalarPtr]:
        """Binds `variable` of the tables of 2^log2n scalars behind the pointers to r (MsmContext.scalars_bind).  Without
        options the top variable is bound in place and every pointer then holds 2^(log2n - 1) scalars; options {"dst": [...]}
        names as many destination pointers, which may not be the sources.  Returns the pointers that hold the result."""
        options = options or {}
        n, h = 1 << log2n, 1 << (log2n - 1)
        srcs = [self._scalar_dev(p, n, "scalarsBind") for p in ptrs]
        dst_ptrs = options.get("dst")
        if dst_ptrs is None:
            if variable != log2n - 1:
                raise MsmError(_lib.MSM_ERR_ARG, "scalarsBind: only the top variable is bound in place; name options.dst")
            self._ctx.scalars_bind(srcs, srcs, log2n, variable, r)
            for p in ptrs:
                p.n = h
            return list(ptrs)
        dsts = [self._scalar_dev(p, h, "scalarsBind", alloc=True) for p in dst_ptrs]
        self._ctx.scalars_bind(dsts, srcs, log2n, variable, r)
        return list(dst_ptrs)

    def scalarsEq(self, r, s=None) -> ScalarPtr:
        """A new scalar pointer holding the table eq(r, .) scaled by s, 2^len(r) scalars (MsmContext.scalars_eq)."""
        r = list(r)
        n = 1 << len(r)
        ptr = ScalarPtr(self._ctx, size=32 * n)
        self._ctx.scalars_eq(self._scalar_dev(ptr, n, "scalarsEq", alloc=True), r, s)
        return ptr

    matrixFromTriplets = staticmethod(matrix_from_triplets)

    def matrixCreate(self, matrix: CsrMatrix, options: Optional[Dict] = None) -> int:
        """A resident sparse matrix from a CsrMatrix (matrixFromTriplets); returns its id (MsmContext.matrix_create).
        options: {"transpose": bool}."""
        return self._ctx.matrix_create(matrix, transpose=bool((options or {}).get("transpose", False)))

    def matrixDestroy(self, matrixId: int) -> None:
        self._ctx.matrix_destroy(matrixId)

    def matrixInfo(self, matrixId: int) -> Dict[str, int]:
        return self._ctx.matrix_info(matrixId)

    def scalarsMatvec(self, matrixId: int, dstPtr: ScalarPtr, xPtr: ScalarPtr, options: Optional[Dict] = None) -> ScalarPtr:
        """dstPtr = alpha M xPtr (+ dstPtr) mod q (MsmContext.scalars_matvec).  options: {"alpha": int or 32 bytes,
        "accumulate": bool}.  Without accumulate dstPtr gets a buffer of `rows` scalars if it has none that large."""
        options = options or {}
        info = self._ctx.matrix_info(matrixId)
        acc = bool(options.get("accumulate", False))
        x = self._scalar_dev(xPtr, info["cols"] if info["nnz"] else 0, "scalarsMatvec")
        d = self._scalar_dev(dstPtr, info["rows"], "scalarsMatvec", alloc=not acc)
        self._ctx.scalars_matvec(matrixId, d, x, options.get("alpha"), acc)
        return dstPtr

    def foldScalars(self, scalarPtr: ScalarPtr, a, b) -> ScalarPtr:
        """The in-place fold of the scalars behind scalarPtr: v[i] <- a * v[i] + b * v[i + n/2]; the pointer then holds n/2
        scalars (MsmContext.fold_scalars)."""
        dev = self._scalar_dev(scalarPtr, scalarPtr.n, "foldScalars")
        scalarPtr.n = self._ctx.fold_scalars(dev, scalarPtr.n, a, b)
        return scalarPtr

    def msmProjective(self, scalarPtr: ScalarPtr, pointPtr: PointPtr, N: int, options: Optional[Dict] = None) -> Dict:
        """`msmProjective` (src/parallel.ts:69-87: msmBasic over projective points): signed windows of the whole scalar,
        no endomorphism split, K = ceil((b + 1) / c) with b = bit length of q (src/msm-basic.ts:56-59).  The bucket sums
        still come from the batched-affine tree; the value is the same group element either way."""
        options = dict(options or {})
        options["noGlv"] = True
        return self.msm(scalarPtr, pointPtr, N, False, options)

    def msmUnsafe(self, scalarPtr: ScalarPtr, pointPtr: PointPtr, N: int, verboseTiming: bool = False,
                  options: Optional[Dict] = None) -> Dict:
        """`msmUnsafe` (src/msm-batched-affine.ts:587-598). The GPU kernels always handle the edge cases."""
        options = dict(options or {})
        options["useSafeAdditions"] = False
        return self.msm(scalarPtr, pointPtr, N, verboseTiming, options)


class _ValuePtr:
    """Stand-in for a wasm pointer of the reference (`Field.getPointer(size)`): holds the value written through it."""

    def __init__(self, size: int = 0):
        self.size, self.value = size, None


class _FieldShim:
    """`Curve.Field.getPointer / getPointers` as the reference's callers use them around an MSM."""

    @staticmethod
    def getPointer(size: int = 0) -> _ValuePtr:
        return _ValuePtr(size)

    @staticmethod
    def getPointers(n: int, size: int = 0) -> List[_ValuePtr]:
        return [_ValuePtr(size) for _ in range(n)]


class _AffineShim:
    """`Curve.Affine.toBigint(ptr)` (src/curve-affine.ts:220-233) -> {"x", "y", "isZero"}; the value behind the pointer is
    already canonical affine here."""

    def __init__(self, coord_bytes: int):
        self.size = 2 * coord_bytes + 4

    @staticmethod
    def toBigint(ptr) -> Dict:
        r = ptr.value if isinstance(ptr, _ValuePtr) else ptr
        return {"x": r.x, "y": r.y, "isZero": bool(r.isZero)}


class _ProjectiveShim:
    """`Curve.Projective.toAffine(scratch, affinePtr, result)` (src/curve-projective.ts:335-349): the reference's callers pass
    the `result` of `Parallel.msm` through it (scripts/msm-weierstrass.ts:89-91).  The library has normalised the sum already,
    so this only stores it behind the pointer."""

    def __init__(self, coord_bytes: int):
        self.size = 3 * coord_bytes + 4

    @staticmethod
    def toAffine(_scratch, affinePtr: _ValuePtr, result: AffineResult) -> None:
        affinePtr.value = result


class _TeCurveShim:
    """`Curve.Curve.toBigint(result)` of the twisted-Edwards module -> extended point {"X", "Y", "Z", "T"}
    (scripts/msm-twisted-edwards.ts:87, scripts/zprize23/submission.ts:33)."""

    def __init__(self, p: int):
        self.p = p

    def toBigint(self, result) -> Dict:
        r = result.value if isinstance(result, _ValuePtr) else result
        return {"X": r.x, "Y": r.y, "Z": 1, "T": r.x * r.y % self.p}


class _TeBigintShim:
    """`Curve.Bigint.toAffine(P)` (src/bigint/twisted-edwards.ts): {"X", "Y", "Z", ...} -> {"x", "y"}."""

    def __init__(self, p: int):
        self.p = p

    def toAffine(self, P: Dict) -> Dict:
        zi = pow(P["Z"], -1, self.p)
        return {"x": P["X"] * zi % self.p, "y": P["Y"] * zi % self.p}


class Weierstrass:
    """Curve module as `Weierstraß.create(params)` returns it (src/parallel.ts:147-160), MSM path only."""

    def __init__(self, params: WeierstrassParams, device: int = 0, devices: Optional[Sequence[int]] = None):
        """`devices`: a device list instead of one device -- every device holds the whole point set and `Parallel.msm` runs
        all windows on each device's share of the points (by points, the default; `by_window=True` on the context's run calls
        shards by scalar window instead; msm_ctx_create_multi); the counterpart of the reference's thread count,
        src/parallel.ts:40-66."""
        if params.label not in _WEIERSTRASS_CURVE_IDS:
            raise MsmError(_lib.MSM_ERR_ARG, f"curve {params.label!r} has no device constants "
                                             f"(have {sorted(_WEIERSTRASS_CURVE_IDS)})")
        self.params = params
        self.context = MsmContext(_WEIERSTRASS_CURVE_IDS[params.label], device, devices=devices)
        self.Parallel = _Parallel(self.context, params)
        self.Field = _FieldShim()
        self.Affine = _AffineShim(self.context.coord_bytes)
        self.Projective = _ProjectiveShim(self.context.coord_bytes)

    @classmethod
    def create(cls, params: WeierstrassParams, device: int = 0, devices: Optional[Sequence[int]] = None) -> "Weierstrass":
        return cls(params, device, devices)


def create_weierstrass(params: WeierstrassParams = BLS12_377_PARAMS, device: int = 0,
                       devices: Optional[Sequence[int]] = None) -> Weierstrass:
    return Weierstrass.create(params, device, devices)


class TwistedEdwards:
    """Curve module as `TwistedEdwards.create(params)` returns it (src/parallel.ts:179-289), MSM path only:
    `Parallel.msm` is `msmBasic` (src/msm-basic.ts:45-164) on extended points."""

    def __init__(self, params: TwistedEdwardsParams, device: int = 0, devices: Optional[Sequence[int]] = None):
        if params.label != "ed-on-bls12-377":
            raise MsmError(_lib.MSM_ERR_ARG, f"curve {params.label!r} has no device constants (only ed-on-bls12-377)")
        self.params = params
        self.context = MsmContext(_lib.CURVE_ED_ON_BLS12_377, device, devices=devices)
        self.Parallel = _Parallel(self.context, params)
        self.Field = _FieldShim()
        self.Curve = _TeCurveShim(params.modulus)
        self.Bigint = _TeBigintShim(params.modulus)

    @classmethod
    def create(cls, params: TwistedEdwardsParams, device: int = 0, devices: Optional[Sequence[int]] = None) -> "TwistedEdwards":
        return cls(params, device, devices)


class _LazyCurve:
    """`BLS12377` of src/concrete/bls12-377.ts: created on first use (needs a GPU)."""

    def __init__(self, params: WeierstrassParams):
        self._params = params
        self._curve: Optional[Weierstrass] = None

    def _get(self) -> Weierstrass:
        if self._curve is None:
            self._curve = Weierstrass.create(self._params)
        return self._curve

    def __getattr__(self, name):
        return getattr(self._get(), name)


Weierstraß = Weierstrass   # the reference's spelling, src/parallel.ts:40


def startThreads(n: Optional[int] = None) -> None:
    """`startThreads(n)` of src/parallel.ts:291-309, which the reference's callers run before any MSM
    (scripts/msm-weierstrass.ts:14, src/msm.test.ts:23).  The worker pool it starts is replaced by the GPU grid: nothing to do."""


def stopThreads() -> None:
    """`stopThreads()` of src/parallel.ts:317-320: nothing to stop (contexts are closed through their curve objects)."""


BLS12377 = _LazyCurve(BLS12_377_PARAMS)
BLS12381 = _LazyCurve(BLS12_381_PARAMS)  # src/concrete/bls12-381.ts


def compute_msm_ed(inputPoints, inputScalars, curve: Optional[TwistedEdwards] = None) -> Dict[str, int]:
    """ZPrize entry point for the twisted Edwards curve, scripts/zprize23/submission.ts:19-60.

    inputPoints: bytes (n x 64, x || y little-endian) or a list of {"x", "y", ...} dicts (z = 1 assumed);
    inputScalars: bytes (n x 32) or a list of ints.  Returns {"x": int, "y": int} (the identity is (0, 1))."""
    cv = curve or TwistedEdwards.create(ED_ON_BLS12_377_PARAMS)
    if isinstance(inputScalars, (bytes, bytearray, memoryview)):
        sbytes = bytes(inputScalars)
    else:
        sbytes = b"".join(int(s).to_bytes(32, "little") for s in inputScalars)
    n = len(sbytes) // 32
    if isinstance(inputPoints, (bytes, bytearray, memoryview)):
        pbytes = bytes(inputPoints)
    else:
        pbytes = b"".join(int(P["x"]).to_bytes(32, "little") + int(P["y"]).to_bytes(32, "little") for P in inputPoints)
    par = cv.Parallel
    with par.getPointer(len(pbytes)) as pp, par.getScalarPointer(len(sbytes)) as sp:   # freed on every path, errors included
        par.pointsFromBytes(pp, pbytes, n)
        par.scalarsFromBytes(sp, sbytes, n)
        res = par.msm(sp, pp, n)["result"]
    return {"x": res.x, "y": res.y}


def compute_msm(inputPoints, inputScalars, curve=None) -> Dict[str, int]:
    """ZPrize entry point, scripts/zprize23/submission-bls377.ts:20-65.

    inputPoints: bytes (x || y little-endian at the curve's coordinate width: n x 96, or n x 64 on a 32-byte curve) or a list of
    {"x", "y", "isZero"} dicts; inputScalars: bytes (n x 32 little-endian) or a list of ints.  Returns {"x": int, "y": int}.
    curve: a curve module (Weierstrass.create), or curve parameters (BN254, PALLAS_PARAMS, ...) for a module that lives for
    this call; default BLS12-377.
    """
    if isinstance(curve, WeierstrassParams):
        cv = Weierstrass.create(curve)
        try:
            return compute_msm(inputPoints, inputScalars, cv)
        finally:
            cv.context.close()
    cv = curve or BLS12377._get()
    wb = cv.Parallel._wire_bytes
    if isinstance(inputScalars, (bytes, bytearray, memoryview)):
        sbytes = bytes(inputScalars)
    else:
        sbytes = b"".join(int(s).to_bytes(32, "little") for s in inputScalars)
    n = len(sbytes) // 32
    if isinstance(inputPoints, (bytes, bytearray, memoryview)):
        pbytes = bytes(inputPoints)
    else:
        chunks = []
        for P in inputPoints:
            if P.get("isZero"):
                chunks.append(b"\0" * (2 * wb))
            else:
                chunks.append(int(P["x"]).to_bytes(wb, "little") + int(P["y"]).to_bytes(wb, "little"))
        pbytes = b"".join(chunks)
    par = cv.Parallel
    with par.getPointer(len(pbytes)) as pp, par.getScalarPointer(len(sbytes)) as sp:   # freed on every path, errors included
        par.pointsFromBytes(pp, pbytes, n)
        par.scalarsFromBytes(sp, sbytes, n)
        same = n > 1 and pbytes[: 2 * wb] == pbytes[2 * wb : 4 * wb]
        out = par.msm(sp, pp, n) if same else par.msmUnsafe(sp, pp, n)
        res = out["result"]
    return {"x": res.x, "y": res.y}
