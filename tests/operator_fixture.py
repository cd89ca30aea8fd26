"""What the GPU tests of the resident operators share: the crafted inputs (non-canonical elements among random residues) and one
fixture class -- a context per curve whose vectors sit `pad` elements into a sentinel-fenced allocation."""
import ctypes

import degenerate_inputs as D
from oracle import msm_oracle as O

TOP = (1 << 256) - 1
SENTINEL = b"\xa5" * 32


def to_bytes(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def edges(q):
    return [0, 1, q - 1, q, q + 1, TOP]


def with_specials(vals, special, start=3):
    """puts special[0], special[1], ... into every seventh place of an already drawn list, from `start` on"""
    for i in range(start, len(vals), 7):
        vals[i] = special[(i // 7) % len(special)]
    return vals


def mixed(prefix, cv, tag, n, start=3):
    """n elements below 2^256: random residues (drawn under the test file's `prefix`) with q, q + 1, 2^256 - 1 and 0 in every
    seventh place from `start` on"""
    q = cv.q
    return with_specials(O.prng_ints(f"{prefix}/{cv.name}/{tag}", n, q), (q, q + 1, TOP, 0), start)


class OperatorFixture:
    """One context per curve; vectors live `pad` (odd) elements inside allocations that end in a sentinel element."""

    def __init__(self, name):
        from montgomery_amd.api import MsmContext

        self.name, self.cv = name, D.CURVE_TABLE[name]
        self.q = self.cv.q
        self.ctx = MsmContext(self.cv.cid)
        self.bufs = []

    def vector(self, vals_or_n, pad=3):
        """device address of a vector holding vals (or n sentinel elements), `pad` elements into its allocation, one sentinel behind"""
        raw = to_bytes(vals_or_n) if not isinstance(vals_or_n, int) else SENTINEL * vals_or_n
        base = self.ctx.device_alloc(32 * pad + len(raw) + 32)
        self.bufs.append(base)
        self.ctx.device_upload(base, SENTINEL * pad + raw + SENTINEL)
        return base + 32 * pad

    def read(self, ptr, n):
        return O.scalars_from_bytes(self.ctx.device_download(ptr, 32 * n)) if n else []

    def raw(self, ptr, n):
        return self.ctx.device_download(ptr, 32 * n)

    def is_sentinel(self, ptr):
        return self.ctx.device_download(ptr, 32) == SENTINEL

    def fenced(self, ptr, n):
        return self.is_sentinel(ptr - 32) and self.is_sentinel(ptr + 32 * n)

    def free(self, *ptrs, pad=3):
        for ptr in ptrs:
            base = ptr - 32 * pad
            self.bufs.remove(base)
            self.ctx.device_free(base)

    def point(self, res):
        """a result in the form Curve.scale_g gives"""
        return (res.x, res.y) if self.cv.te else res.as_tuple()

    def last(self, entry, cap):
        """the report of an msm_test_last_* entry of the library: as many words as it says it wrote"""
        out = (ctypes.c_int32 * cap)()
        count = getattr(self.ctx._lib, entry)(self.ctx._h, out, cap)
        assert count >= 0, (entry, count)
        return list(out[:count])

    def set(self, entry, *args):
        """an msm_test_set_* entry of the library, which must accept"""
        assert getattr(self.ctx._lib, entry)(self.ctx._h, *args) == 0

    def close(self):
        for b in self.bufs:
            self.ctx.device_free(b)
        self.ctx.close()
