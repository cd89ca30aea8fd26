"""Narrow-scalar MSM through the N-API addon and the JS facade: the exports (no GPU), and js/test-narrow.js (`-m gpu`)."""
import pytest

from napi_support import assert_exports, run_js


def test_addon_and_facade_export_the_narrow_entries():
    assert_exports(("msmNarrow", "msmBatchNarrow", "scalarBits"))


@pytest.mark.gpu
def test_js_msm_narrow_equals_msm():
    run_js("test-narrow.js", 600)
