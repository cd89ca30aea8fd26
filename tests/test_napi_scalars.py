"""The resident scalar-vector operations through the N-API addon and the JS facade: the exports (no GPU), and
js/test-scalars.js (`-m gpu`)."""
import pytest

from napi_support import assert_exports, run_js

NAMES = ("deviceDownload", "scalarsLincomb", "scalarsMul", "scalarsInner", "scalarsPowers")


def test_addon_and_facade_export_the_scalar_entries():
    assert_exports(NAMES, facade=NAMES[1:] + ("foldScalars",), hip_calls=("deviceDownload",))


@pytest.mark.gpu
def test_js_scalars_equal_bigint_arithmetic():
    run_js("test-scalars.js", 600)
