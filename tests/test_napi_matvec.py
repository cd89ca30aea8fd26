"""Resident sparse matrices and the matrix-vector product through the N-API addon and the JS facade: the exports (no GPU), and
js/test-matvec.js (`-m gpu`)."""
import pytest

from napi_support import assert_exports, run_js

NAMES = ("matrixCreate", "matrixDestroy", "matrixInfo", "scalarsMatvec")


def test_addon_and_facade_export_the_matrix_entries():
    assert_exports(NAMES, facade=NAMES + ("matrixFromTriplets",), hip_calls=NAMES)


@pytest.mark.gpu
def test_js_matvec_equals_bigint_arithmetic():
    run_js("test-matvec.js", 600)
