"""The resident scans through the N-API addon and the JS facade: the exports (no GPU), and js/test-scans.js (`-m gpu`)."""
import pytest

from napi_support import assert_exports, run_js

NAMES = ("scalarsScan", "scalarsInverse", "scalarsDivLinear")


def test_addon_and_facade_export_the_scan_entries():
    assert_exports(NAMES, hip_calls=NAMES)


@pytest.mark.gpu
def test_js_scans_equal_bigint_arithmetic():
    run_js("test-scans.js", 600)
