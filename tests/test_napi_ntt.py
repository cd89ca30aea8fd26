"""The resident NTT through the N-API addon and the JS facade: the exports (no GPU), and js/test-ntt.js (`-m gpu`)."""
import pytest

from napi_support import assert_exports, run_js

NAMES = ("scalarsNtt", "scalarsRootOfUnity", "scalarsNttMaxLog2n")


def test_addon_and_facade_export_the_ntt_entries():
    assert_exports(NAMES, facade=NAMES[:2], hip_calls=NAMES[:2])


@pytest.mark.gpu
def test_js_ntt_equals_bigint_arithmetic():
    run_js("test-ntt.js", 600)
