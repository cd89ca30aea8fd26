"""The resident sumcheck through the N-API addon and the JS facade: the exports (no GPU), and js/test-sumcheck.js (`-m gpu`)."""
import pytest

from napi_support import assert_exports, run_js

NAMES = ("scalarsSumcheckRound", "scalarsBind", "scalarsEq")


def test_addon_and_facade_export_the_sumcheck_entries():
    assert_exports(NAMES, hip_calls=NAMES)


@pytest.mark.gpu
def test_js_sumcheck_equals_bigint_arithmetic():
    run_js("test-sumcheck.js", 600)
