"""What the tests of the host shims (tests/csrc/lib*_host.so) share: the loader, and field elements as little-endian arrays of
32-bit words for ctypes."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_library(stem):
    """tests/csrc/lib<stem>.so, built when it is not there.  The argtypes are the caller's to declare."""
    from conftest import build_if_missing

    path = f"tests/csrc/lib{stem}.so"
    build_if_missing(path, path)
    return C.CDLL(os.path.join(ROOT, path))


def words(v, n=8):
    return (C.c_uint32 * n)(*[(v >> (32 * j)) & 0xFFFFFFFF for j in range(n)])


def vec(vals):
    return (C.c_uint32 * (8 * max(len(vals), 1)))(*[(v >> (32 * j)) & 0xFFFFFFFF for v in vals for j in range(8)])


def value(w, i=0, n=8):
    return sum(int(w[n * i + j]) << (32 * j) for j in range(n))
