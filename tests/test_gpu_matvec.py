"""Resident sparse matrices and dst = alpha M x (+ dst) on the GPU: msm_matrix_create / _destroy / _info and msm_scalars_matvec.
`-m gpu`.

Expected values are Python integers mod cv.q; every comparison is bit-exact.  Vectors sit at an odd 32-byte offset inside their
allocation and end in a sentinel element; x and the coefficients carry non-canonical elements (q, q + 1, 2^256 - 1) and zeros
among the random ones.  Row lengths: the ladder 0, 4, 5, 63, 64, 65, 128, 129, 5 * 64 + 3 of the CPU plan test, run at the forced
thresholds (4, 64), (1, 1) and (4, 96) and, with rows either side of them, at the defaults the library reports."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degenerate_inputs as D  # noqa: E402
import operator_fixture as F  # noqa: E402
from operator_fixture import TOP, OperatorFixture, edges, to_bytes  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

LADDER = (0, 4, 5, 63, 64, 65, 128, 129, 5 * 64 + 3)
GEOMETRIES = ((4, 64), (1, 1), (4, 96), (0, 0))   # (0, 0): the defaults


def u32_bytes(vals):
    return b"".join(v.to_bytes(4, "little") for v in vals)


def mixed(rng, q, n):
    """n elements below 2^256: random ones with q, q + 1, 2^256 - 1 and 0 in every seventh place"""
    return F.with_specials([rng.randrange(q) for _ in range(n)], (q, q + 1, TOP, 0))


def csr(rows):
    """rows: per row a list of (col, value) or of col -> (row_ptr, col, val or None)"""
    rp, col, val = [0], [], []
    for r in rows:
        for e in r:
            if isinstance(e, tuple):
                col.append(e[0])
                val.append(e[1])
            else:
                col.append(e)
        rp.append(len(col))
    return rp, col, (val if val else None) if col else None


def product_ref(rows, x, q, alpha=None, old=None):
    out = []
    for i, r in enumerate(rows):
        s = sum((e[1] * x[e[0]]) if isinstance(e, tuple) else x[e] for e in r)
        out.append(((1 if alpha is None else alpha) * s + (old[i] if old is not None else 0)) % q)
    return out


def plan_counts(lens, short_max, part_len):
    long_rows = [n for n in lens if n > short_max]
    return len(long_rows), sum(-(-n // part_len) for n in long_rows)


def transpose_rows(rows, cols):
    t = [[] for _ in range(cols)]
    for i, r in enumerate(rows):
        for e in r:
            t[e[0] if isinstance(e, tuple) else e].append((i, e[1]) if isinstance(e, tuple) else i)
    return t


class Fix(OperatorFixture):
    def __init__(self, name):
        super().__init__(name)
        self.rng = random.Random(f"matvec/{name}")

    def blob(self, data):
        """an unfenced allocation that holds `data` as it is"""
        base = self.ctx.device_alloc(max(len(data), 32))
        self.bufs.append(base)
        if data:
            self.ctx.device_upload(base, data)
        return base

    def geometry(self, short_max, part_len):
        self.set("msm_test_set_matvec_geometry", short_max, part_len)

    def last(self):
        out = super().last("msm_test_last_matvec", 5)
        assert len(out) == 5
        return out

    def matrix(self, rows, cols, geometry=(0, 0), transpose=False):
        self.geometry(*geometry)
        rp, col, val = csr(rows)
        mid = self.ctx.matrix_create(len(rows), cols, rp, col, val, transpose=transpose)
        self.geometry(0, 0)
        return mid

    def product(self, mid, n_rows, x, alpha=None, old=None):
        """runs one product into a fresh dst (preloaded with `old` under ACCUMULATE); -> the rows; checks the sentinels and x"""
        xp = self.vector(x) if not isinstance(x, int) else x
        dp = self.vector(old if old is not None else n_rows, pad=5)
        self.ctx.scalars_matvec(mid, dp, xp, alpha, accumulate=old is not None)
        assert self.is_sentinel(dp - 32) and self.is_sentinel(dp + 32 * n_rows)
        if not isinstance(x, int):
            assert self.read(xp, len(x)) == x
        return self.read(dp, n_rows)

    def check(self, rows, cols, x, geometry=(0, 0), alpha=None, old=None, what=None):
        mid = self.matrix(rows, cols, geometry)
        got = self.product(mid, len(rows), x, alpha, old)
        assert got == product_ref(rows, x, self.q, alpha, old), (self.name, geometry, what)
        last = self.last()
        self.ctx.matrix_destroy(mid)
        return last

    def random_rows(self, lens, cols, ones=False):
        rng, q = self.rng, self.q
        out = []
        for n in lens:
            if ones:
                out.append([rng.randrange(cols) for _ in range(n)])
            else:
                vals = mixed(rng, q, n)
                out.append([(rng.randrange(cols), v) for v in vals])
        return out


@pytest.fixture(scope="module", params=D.NAMES)
def f7(request):
    f = Fix(request.param)
    yield f
    f.close()


@pytest.fixture(scope="module")
def f1():
    f = Fix("bls377")
    yield f
    f.close()


# ---------------------------------------------------------------------------------------------- 1: edges

def test_no_entries_one_entry_one_long_row(f1):
    f, q = f1, f1.q
    # nnz = 0 over 5 rows: zeros written; with ACCUMULATE dst is canonicalised only.  x is not read: none is given
    mid = f.ctx.matrix_create(5, 3, [0] * 6, [], None)
    assert f.product(mid, 5, 0) == [0] * 5 and f.last()[2:] == [0, 0, 1]
    old = [q + 1, TOP, 0, q, 7]
    assert f.product(mid, 5, 0, old=old) == [v % q for v in old]
    assert f.product(mid, 5, 0, alpha=q - 1, old=old) == [v % q for v in old]
    assert f.ctx.matrix_info(mid)["nnz"] == 0
    f.ctx.matrix_destroy(mid)
    # no rows at all: nothing is launched, nothing is written
    mid = f.ctx.matrix_create(0, 3, [0], [], None)
    assert f.product(mid, 0, [1, 2, 3]) == [] and f.last()[4] == 0
    f.ctx.matrix_destroy(mid)
    # 1 x 1 with one entry
    for c, x in ((5, 7), (q + 1, TOP), (0, 9)):
        f.check([[(0, c)]], 1, [x], what="1x1")
    # one row of 1000 entries: a single long row under the defaults if they put it there, and always under (4, 64)
    rows = f.random_rows([1000], 17)
    x = mixed(f.rng, q, 17)
    assert f.check(rows, 17, x, (4, 64))[:5] == [4, 64, 1, 16, 3]
    f.check(rows, 17, x)


@pytest.mark.parametrize("n_rows", (255, 256, 257))
def test_rows_around_a_block(f1, n_rows):
    f = f1
    rows = f.random_rows([(3 * i) % 5 for i in range(n_rows)], 40)
    rows[n_rows - 1] = f.random_rows([9], 40)[0]       # the last row is long at (4, 64)
    x = mixed(f.rng, f.q, 40)
    assert f.check(rows, 40, x, (4, 64))[2:] == [1, 1, 3]
    last = f.check(rows, 40, x)
    assert last[4] == (3 if 9 > last[0] else 1)


# ---------------------------------------------------------------------------------------------- 2: the length ladder

def test_the_length_ladder_at_forced_and_default_geometries(f7):
    f, q = f7, f7.q
    cols = 50
    rows = f.random_rows(LADDER, cols)
    x = mixed(f.rng, q, cols)
    for geo in GEOMETRIES:
        last = f.check(rows, cols, x, geo, what="ladder")
        short_max, part_len = last[:2]
        if geo != (0, 0):
            assert (short_max, part_len) == geo
        n_long, n_parts = plan_counts(LADDER, short_max, part_len)
        assert last[2:] == [n_long, n_parts, 3 if n_long else 1], (f.name, geo, last)
    assert plan_counts(LADDER, 4, 64) == (7, 16) and plan_counts(LADDER, 1, 1) == (8, sum(LADDER)) and plan_counts(LADDER, 4, 96) == (7, 12)
    # rows either side of the default thresholds, read from the report
    short_max, part_len = last[:2]
    assert short_max >= 1 and part_len >= 1
    lens = [short_max - 1, short_max, short_max + 1, part_len - 1, part_len, part_len + 1, 2 * part_len, 2 * part_len + 1]
    rows = f.random_rows(lens, cols)
    last = f.check(rows, cols, x, what="default thresholds")
    n_long, n_parts = plan_counts(lens, short_max, part_len)
    assert n_long >= 5 and last == [short_max, part_len, n_long, n_parts, 3]


def test_the_ladder_in_the_all_ones_form(f1):
    f = f1
    rows = f.random_rows(LADDER, 50, ones=True)
    x = mixed(f.rng, f.q, 50)
    for geo in GEOMETRIES:
        f.check(rows, 50, x, geo, alpha=None if geo[0] != 1 else f.q - 2, what="ones ladder")


# ---------------------------------------------------------------------------------------------- 3: same bytes at every geometry

def test_a_random_matrix_gives_the_same_bytes_at_four_geometries(f1):
    f, q, rng = f1, f1.q, f1.rng
    n, nnz = 1 << 12, 1 << 14
    rows = [[] for _ in range(n)]
    vals = mixed(rng, q, nnz)
    for j in range(nnz):
        r = rng.randrange(n) if j % 16 else 77          # row 77 takes a sixteenth of the entries: about 1000
        rows[r].append((rng.randrange(n), vals[j]))
    x = mixed(rng, q, n)
    want = product_ref(rows, x, q)
    xp = f.vector(x)
    seen = set()
    for geo in ((0, 0), (1, 1), (4, 64), (2, 7)):
        mid = f.matrix(rows, n, geo)
        dp = f.vector(n, pad=5)
        f.ctx.scalars_matvec(mid, dp, xp)
        raw = f.ctx.device_download(dp, 32 * n)
        assert O.scalars_from_bytes(raw) == want, geo
        seen.add(raw)
        assert f.last()[2] >= 1
        f.ctx.matrix_destroy(mid)
    assert len(seen) == 1


# ---------------------------------------------------------------------------------------------- 4: edge operands

def test_edge_coefficients_against_edge_x_entries(f7):
    f, q = f7, f7.q
    E = edges(q)
    x = E + [3]
    rows = [[(j, c)] for c in E for j in range(6)]                   # one row per pairing
    rows.append([(j, c) for c in E for j in range(6)])               # and one row holding all of them
    for geo in ((0, 0), (4, 8)):
        f.check(rows, 7, x, geo, what="edges")
        f.check(rows, 7, x, geo, alpha=q - 1, old=(E * 7)[:37], what="edges, alpha and old")
    ones = [[j] for j in range(6)] + [list(range(6)) * 3]
    f.check(ones, 7, x, (4, 8), old=E + [TOP], what="edges, all ones")


# ---------------------------------------------------------------------------------------------- 5: row content

def test_unsorted_and_repeated_columns_one_column_and_the_last_column(f1):
    f, q = f1, f1.q
    cols = 33
    x = mixed(f.rng, q, cols)
    rows = [
        [(5, 2), (1, 3), (5, 4), (0, 5), (5, q - 1), (1, TOP)],      # unsorted, column 5 three times
        [(cols - 1, 9)],                                              # the last column
        [(cols - 1, 1), (0, 1), (cols - 1, 1)],
        [(7, v) for v in mixed(f.rng, q, 70)],                        # every entry on one column: long at (4, 64)
        [],
    ]
    for geo in ((0, 0), (4, 64), (1, 1)):
        f.check(rows, cols, x, geo, what="row content")
    f.check([[7] * 70, [cols - 1], [5, 1, 5, 0]], cols, x, (4, 64), what="row content, all ones")


# ---------------------------------------------------------------------------------------------- 6: the all-ones form

def test_a_permutation_gathers_and_rows_sum(f1):
    f, q, rng = f1, f1.q, f1.rng
    n = 1000
    perm = list(range(n))
    rng.shuffle(perm)
    x = mixed(rng, q, n)
    mid = f.ctx.matrix_create(n, n, list(range(n + 1)), perm, None)
    assert f.product(mid, n, x) == [x[p] % q for p in perm]
    info = f.ctx.matrix_info(mid)
    assert (info["rows"], info["cols"], info["nnz"]) == (n, n, n) and 4 * n <= info["bytes"] < 36 * n
    f.ctx.matrix_destroy(mid)
    # row sums: row i adds the elements [10 i, 10 i + 10); one row adds everything
    rows = [list(range(10 * i, 10 * i + 10)) for i in range(n // 10)] + [list(range(n))]
    got = f.check(rows, n, x, what="row sums")
    assert got[2] >= 1


# ---------------------------------------------------------------------------------------------- 7: alpha and ACCUMULATE

def test_alpha_and_accumulate(f7):
    f, q, rng = f7, f7.q, f7.rng
    lens = [0, 1, 2, 3, 4, 5, 9, 70, 1]
    cols = 20
    rows = f.random_rows(lens, cols)
    x = mixed(rng, q, cols)
    old = [q, TOP, 0, q + 1, rng.randrange(q), q - 1, 1, TOP - 1, rng.randrange(1 << 256)]   # raw values, some >= q
    mid = f.matrix(rows, cols, (4, 64))
    for alpha in (None, 0, 1, q - 1, rng.randrange(q)):
        assert f.product(mid, len(rows), x, alpha) == product_ref(rows, x, q, alpha), (f.name, alpha)
        assert f.product(mid, len(rows), x, alpha, old) == product_ref(rows, x, q, alpha, old), (f.name, alpha, "accumulate")
    f.ctx.matrix_destroy(mid)


# ---------------------------------------------------------------------------------------------- 8: transposition

def test_transposition_against_the_model_and_the_adjoint_identity(f1):
    f, q, rng = f1, f1.q, f1.rng
    n_rows, n_cols = 90, 37
    rows = f.random_rows([rng.choice((0, 1, 2, 3, 6)) for _ in range(n_rows)], n_cols)
    for i, r in enumerate(rows):
        r.insert(i % (len(r) + 1), (0, rng.randrange(1 << 256)))     # column 0 is hit by every row
    t_rows = transpose_rows(rows, n_cols)
    assert len(t_rows[0]) >= n_rows
    x, y = mixed(rng, q, n_cols), mixed(rng, q, n_rows)
    m = f.matrix(rows, n_cols, (4, 64))
    mt = f.matrix(rows, n_cols, (4, 64), transpose=True)
    info = f.ctx.matrix_info(mt)
    assert (info["rows"], info["cols"], info["nnz"]) == (n_cols, n_rows, sum(len(r) for r in rows))
    xp, yp, mx, mty = f.vector(x), f.vector(y), f.vector(n_rows), f.vector(n_cols)
    f.ctx.scalars_matvec(m, mx, xp)
    f.ctx.scalars_matvec(mt, mty, yp)
    assert f.last()[2] >= 1                                           # the column of every row has become a long row
    assert f.read(mty, n_cols) == product_ref(t_rows, y, q)
    assert f.read(mx, n_rows) == product_ref(rows, x, q)
    # <y, M x> = <M^T y, x>
    lhs, rhs = f.ctx.scalars_inner(yp, mx, n_rows), f.ctx.scalars_inner(mty, xp, n_cols)
    assert lhs == rhs == sum(a * b for a, b in zip(y, product_ref(rows, x, q))) % q
    # the all-ones form transposed: a scatter-add
    idx = [rng.randrange(n_cols) for _ in range(n_rows)]
    g = f.ctx.matrix_create(n_rows, n_cols, list(range(n_rows + 1)), idx, None, transpose=True)
    want = [0] * n_cols
    for i, c in enumerate(idx):
        want[c] = (want[c] + y[i]) % q
    assert f.product(g, n_cols, y) == want
    for mid in (m, mt, g):
        f.ctx.matrix_destroy(mid)


# ---------------------------------------------------------------------------------------------- 9: ownership

def test_device_input_equals_host_input_and_the_matrix_owns_its_arrays(f1):
    f, q, rng = f1, f1.q, f1.rng
    cols = 29
    rows = f.random_rows([0, 3, 1, 80, 2, 5, 0], cols)
    rp, col, val = csr(rows)
    nnz = len(col)
    x = mixed(rng, q, cols)
    want = product_ref(rows, x, q)
    f.geometry(4, 64)
    host = f.ctx.matrix_create(len(rows), cols, rp, col, val)
    # the device arrays at odd offsets: row_ptr and col on 4-byte boundaries, val on a 16-byte one
    d_rp, d_col, d_val = f.blob(bytes(4) + u32_bytes(rp)) + 4, f.blob(bytes(12) + u32_bytes(col)) + 12, f.blob(bytes(16) + to_bytes(val)) + 16
    dev = f.ctx.matrix_create(len(rows), cols, d_rp, d_col, d_val, nnz=nnz, on_device=True)
    ones_dev = f.ctx.matrix_create(len(rows), cols, d_rp, d_col, None, nnz=nnz, on_device=True)
    f.geometry(0, 0)
    assert dev != host and ones_dev not in (dev, host)
    # overwriting the caller's arrays after create changes nothing
    for p, size in ((d_rp, 4 * len(rp)), (d_col, 4 * nnz), (d_val, 32 * nnz)):
        f.ctx.device_upload(p, b"\xff" * size)
    assert f.product(host, len(rows), x) == want
    assert f.product(dev, len(rows), x) == want and f.last()[:4] == [4, 64, 2, 3]
    assert f.product(ones_dev, len(rows), x) == product_ref([[e[0] for e in r] for r in rows], x, q)
    for mid, per in ((host, 36), (dev, 36), (ones_dev, 4)):
        info = f.ctx.matrix_info(mid)
        assert (info["rows"], info["cols"], info["nnz"]) == (len(rows), cols, nnz) and info["bytes"] >= per * nnz
    assert f.ctx.matrix_info(ones_dev)["bytes"] < f.ctx.matrix_info(dev)["bytes"] - 32 * nnz + 1024
    # ids: a destroyed one is gone, and is handed out again
    f.ctx.matrix_destroy(dev)
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError

    for call in (lambda: f.ctx.matrix_info(dev), lambda: f.ctx.matrix_destroy(dev), lambda: f.product(dev, len(rows), x)):
        with pytest.raises(MsmError) as e:
            call()
        assert e.value.code == MSM_ERR_ARG and f"no matrix {dev}" in str(e.value)
    again = f.ctx.matrix_create(1, 1, [0, 1], [0], [3])
    assert again == dev
    for mid in (host, ones_dev, again):
        f.ctx.matrix_destroy(mid)


# ---------------------------------------------------------------------------------------------- 10: refusals

GOOD_RP, GOOD_COL = [0, 2, 2, 5, 6], [3, 0, 1, 1, 4, 2]   # 4 x 5, 6 entries
DEFECTS = (
    # row_ptr, col, the text that names the position and the value
    ([1, 2, 2, 5, 6], GOOD_COL, "row_ptr[0] = 1 but must be 0"),
    ([0, 2, 1, 5, 6], GOOD_COL, "row_ptr[2] = 1 but row_ptr[1] = 2"),
    ([0, 3, 2, 1, 6], GOOD_COL, "row_ptr[2] = 2 but row_ptr[1] = 3"),       # the smallest of two
    ([0, 2, 2, 5, 5], GOOD_COL, "row_ptr[4] = 5 but nnz = 6"),
    ([0, 2, 2, 5, 7], GOOD_COL, "row_ptr[4] = 7 but nnz = 6"),
    (GOOD_RP, [3, 0, 1, 5, 4, 2], "col[3] = 5 but cols = 5"),
    (GOOD_RP, [3, 0, 1, 1, 4, 0xFFFFFFFF], "col[5] = 4294967295 but cols = 5"),
    (GOOD_RP, [9, 0, 8, 1, 7, 2], "col[0] = 9 but cols = 5"),               # the smallest of three
    ([0, 2, 2, 5, 9], [9, 9, 9, 9, 9, 9], "row_ptr[4] = 9 but nnz = 6"),    # row_ptr before col
)


def test_every_csr_defect_is_refused_for_host_and_device_input(f1):
    """A defect test proves a refusal, not a read: every array is as long as the call says, and a bad index is never used."""
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError

    f, q = f1, f1.q
    x = [3, 5, 7, 11, 13]
    good = f.ctx.matrix_create(4, 5, GOOD_RP, GOOD_COL, None)
    want = product_ref([[3, 0], [], [1, 1, 4], [2]], x, q)
    val = to_bytes([2] * 6)
    for rp, col, text in DEFECTS:
        for on_device in (False, True):
            with pytest.raises(MsmError) as e:
                if on_device:
                    f.ctx.matrix_create(4, 5, f.blob(u32_bytes(rp)), f.blob(u32_bytes(col)), f.blob(val), nnz=6, on_device=True)
                else:
                    f.ctx.matrix_create(4, 5, rp, col, val)
            assert e.value.code == MSM_ERR_ARG and "msm_matrix_create: " + text in str(e.value), (rp, col, on_device)
            # no id was created, and the context goes on
            with pytest.raises(MsmError):
                f.ctx.matrix_info(good + 1)
            assert f.product(good, 4, x) == want
    # id_out is untouched
    ident = ctypes.c_int32(-77)
    rp, col = (ctypes.c_uint32 * 5)(0, 2, 2, 5, 6), (ctypes.c_uint32 * 6)(3, 0, 1, 5, 4, 2)
    assert f.ctx._lib.msm_matrix_create(f.ctx._h, 4, 5, 6, rp, col, None, 0, 0, ctypes.byref(ident)) == MSM_ERR_ARG
    assert ident.value == -77
    f.ctx.matrix_destroy(good)


def test_every_other_refusal_leaves_outputs_and_context_as_they_were(f1):
    from montgomery_amd._lib import MSM_ERR_ARG, MSM_ERR_SCALAR, MsmError

    f, q = f1, f1.q
    lib, h, vp = f.ctx._lib, f.ctx._h, ctypes.c_void_p
    x = [3, 5, 7, 11, 13]
    rows = [[3, 0], [], [1, 1, 4], [2], []]                         # 5 x 5, 6 entries: dst and x have the same size
    want = product_ref(rows, x, q)
    rp, col, _ = csr(rows)
    good = f.ctx.matrix_create(5, 5, rp, col, None)
    both = f.vector(x + [0] * 5)                                     # x, then room for a dst right behind it
    xp, dp = both, both + 32 * 5
    ident = ctypes.c_int32(-77)
    c_rp, c_col = (ctypes.c_uint32 * 6)(*rp), (ctypes.c_uint32 * 6)(*col)

    def still_good():
        assert f.read(xp, 5) == x and f.ctx.device_download(dp, 32 * 5) == bytes(32 * 5) and f.is_sentinel(dp + 32 * 5)
        assert f.product(good, 5, xp) == want

    def create_refused(*args):
        assert lib.msm_matrix_create(h, *args, ctypes.byref(ident)) == MSM_ERR_ARG and ident.value == -77, args
        still_good()

    def matvec_refused(code, mid, dst, src, alpha=None, flags=0):
        ab = None if alpha is None else (ctypes.c_uint8 * 32).from_buffer_copy(alpha.to_bytes(32, "little"))
        assert lib.msm_scalars_matvec(h, mid, None if dst is None else vp(dst), None if src is None else vp(src), ab, flags) == code
        assert f.last() == [0] * 5
        still_good()

    # creation: unknown flag bits, TRANSPOSE with on_device, sizes, null and misaligned pointers
    create_refused(5, 5, 6, c_rp, c_col, None, 0, 2)
    create_refused(5, 5, 6, c_rp, c_col, None, 0, 0x80000001)
    d_rp, d_col, d_val = f.blob(u32_bytes(rp)), f.blob(u32_bytes(col)), f.blob(bytes(32 * 6 + 16))
    create_refused(5, 5, 6, vp(d_rp), vp(d_col), None, 1, 1)
    create_refused(1 << 30, 5, 6, c_rp, c_col, None, 0, 0)
    create_refused(5, 1 << 30, 6, c_rp, c_col, None, 0, 0)
    create_refused(5, 5, 1 << 31, c_rp, c_col, None, 0, 0)
    create_refused(5, 5, 6, None, c_col, None, 0, 0)
    create_refused(5, 5, 6, c_rp, None, None, 0, 0)
    create_refused(5, 5, 6, vp(d_rp + 2), vp(d_col), None, 1, 0)
    create_refused(5, 5, 6, vp(d_rp), vp(d_col + 1), None, 1, 0)
    create_refused(5, 5, 6, vp(d_rp), vp(d_col), vp(d_val + 8), 1, 0)
    assert lib.msm_matrix_create(h, 5, 5, 6, c_rp, c_col, None, 0, 0, None) == MSM_ERR_ARG
    still_good()
    # the product: flags, dst equal to x and overlapping it in part, misaligned and null pointers, alpha, ids
    matvec_refused(MSM_ERR_ARG, good, dp, xp, flags=2)
    matvec_refused(MSM_ERR_ARG, good, dp, xp, flags=0x101)
    matvec_refused(MSM_ERR_ARG, good, xp, xp)
    matvec_refused(MSM_ERR_ARG, good, xp + 32, xp)
    matvec_refused(MSM_ERR_ARG, good, xp + 32 * 4, xp)
    matvec_refused(MSM_ERR_ARG, good, xp - 32 * 2, xp)
    matvec_refused(MSM_ERR_ARG, good, dp + 8, xp)
    matvec_refused(MSM_ERR_ARG, good, dp, xp + 4)
    matvec_refused(MSM_ERR_ARG, good, None, xp)
    matvec_refused(MSM_ERR_ARG, good, dp, None)
    matvec_refused(MSM_ERR_SCALAR, good, dp, xp, alpha=q)
    matvec_refused(MSM_ERR_SCALAR, good, dp, xp, alpha=TOP)
    for bad_id in (0, -1, good + 1, 1 << 20):
        matvec_refused(MSM_ERR_ARG, bad_id, dp, xp)
        assert lib.msm_matrix_destroy(h, bad_id) == MSM_ERR_ARG
    # and the valid neighbours of what was refused: dst right behind x, alpha = q - 1
    f.ctx.scalars_matvec(good, dp, xp, q - 1)
    assert f.read(dp, 5) == product_ref(rows, x, q, q - 1) and f.read(xp, 5) == x
    f.ctx.matrix_destroy(good)
    with pytest.raises(MsmError):
        f.ctx.matrix_destroy(good)


def test_device_list_contexts_are_refused():
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError
    from montgomery_amd.api import MsmContext

    multi = MsmContext(D.CURVE_TABLE["bls377"].cid, devices=[0, 0])
    try:
        p, d = multi.device_alloc(128), multi.device_alloc(128)
        multi.device_upload(p, bytes(128))
        multi.device_upload(d, bytes(128))
        for call in (lambda: multi.matrix_create(2, 2, [0, 1, 2], [0, 1], None), lambda: multi.matrix_info(1),
                     lambda: multi.matrix_destroy(1), lambda: multi.scalars_matvec(1, d, p)):
            with pytest.raises(MsmError) as e:
                call()
            assert e.value.code == MSM_ERR_ARG and "single-device" in str(e.value)
        assert multi._lib.msm_test_set_matvec_geometry(multi._h, 4, 64) == MSM_ERR_ARG
        assert multi._lib.msm_test_last_matvec(multi._h, (ctypes.c_int32 * 5)(), 5) == -1
        assert multi.device_download(p, 128) == bytes(128) and multi.device_download(d, 128) == bytes(128)
    finally:
        multi.close()


# ---------------------------------------------------------------------------------------------- 11: the whole protocol

def interpolate(evals, x, q):
    total = 0
    for t, y in enumerate(evals):
        num = den = 1
        for u in range(len(evals)):
            if u != t:
                num = num * (x - u) % q
                den = den * (t - u) % q
        total += y * num * pow(den, -1, q)
    return total % q


@pytest.mark.parametrize("name", ("bn254", "pallas"))
def test_an_r1cs_prover_without_moving_a_vector(name):
    """Spartan's two phases over a small R1CS, 2^6 constraints and 2^6 variables: A z, B z, C z from msm_scalars_matvec, the outer
    sumcheck of eq(tau, .) (A z . B z - C z) with claim 0, then v = r_A A^T e + r_B B^T e + r_C C^T e in three calls on transposed
    handles with alpha and ACCUMULATE, and <v, z> against the values the bound tables hold."""
    f = Fix(name)
    try:
        q, rng, ctx = f.q, f.rng, f.ctx
        LOG, N = 6, 64
        z = [1] + [rng.randrange(q) for _ in range(N - 1)]
        A = [[(rng.randrange(N), rng.randrange(q)) for _ in range(rng.randrange(1, 5))] for _ in range(N)]
        B = [[(rng.randrange(N), rng.randrange(q)) for _ in range(rng.randrange(1, 5))] for _ in range(N)]
        az, bz = product_ref(A, z, q), product_ref(B, z, q)
        Cm = [[(0, a * b % q)] for a, b in zip(az, bz)]              # z[0] = 1: C z = A z o B z
        zp = f.vector(z)
        handles, tables = [], []
        for M in (A, B, Cm):
            handles.append((f.matrix(M, N), f.matrix(M, N, transpose=True)))
            tables.append(f.vector(N))
            ctx.scalars_matvec(handles[-1][0], tables[-1], zp)
        assert [f.read(t, N) for t in tables] == [az, bz, [a * b % q for a, b in zip(az, bz)]]
        # the outer sumcheck, the top variable bound in place each round
        tau = [rng.randrange(q) for _ in range(LOG)]
        eqp = f.vector(N)
        ctx.scalars_eq(eqp, tau)
        ptrs = [eqp] + tables
        claim, challenges = 0, []
        for rnd in range(LOG):
            log2n = LOG - rnd
            s = ctx.scalars_sumcheck_round(ptrs, log2n, log2n - 1, "r1cs")
            assert (s[0] + s[1]) % q == claim, (name, rnd)
            r = rng.randrange(q)
            challenges.append(r)
            claim = interpolate(s, r, q)
            ctx.scalars_bind(ptrs, ptrs, log2n, log2n - 1, r)
        e_rx, az_rx, bz_rx, cz_rx = (f.read(p, 1)[0] for p in ptrs)
        assert e_rx * (az_rx * bz_rx - cz_rx) % q == claim
        # the second phase: e = eq(r_x, .), variable j of the index took challenge LOG - 1 - j
        rx = challenges[::-1]
        ep, vptr = f.vector(N), f.vector(N)
        ctx.scalars_eq(ep, rx)
        ra, rb, rc = (rng.randrange(q) for _ in range(3))
        ctx.scalars_matvec(handles[0][1], vptr, ep, ra)
        ctx.scalars_matvec(handles[1][1], vptr, ep, rb, accumulate=True)
        ctx.scalars_matvec(handles[2][1], vptr, ep, rc, accumulate=True)
        assert ctx.scalars_inner(vptr, zp, N) == (ra * az_rx + rb * bz_rx + rc * cz_rx) % q
    finally:
        f.close()
