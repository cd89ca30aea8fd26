"""Indexed (sparse) MSM through the N-API addon and the JS facade: the exports (no GPU), and js/test-indexed.js (`-m gpu`)."""
import pytest

from napi_support import assert_exports, run_js

NAMES = ("msmIndexed", "msmIndexedNarrow")


def test_addon_and_facade_export_the_indexed_entries():
    assert_exports(NAMES)


@pytest.mark.gpu
def test_js_msm_indexed_equals_dense_msm():
    run_js("test-indexed.js", 600)
