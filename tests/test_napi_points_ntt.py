"""The transform over point sets through the N-API addon and the JS facade: the exports (no GPU), and js/test-points-ntt.js
(`-m gpu`)."""
import pytest

from napi_support import assert_exports, run_js

NAMES = ("pointsNtt",)


def test_addon_and_facade_export_the_points_ntt_entry():
    assert_exports(NAMES)


@pytest.mark.gpu
def test_js_points_ntt_equals_the_bigint_transform():
    run_js("test-points-ntt.js", 600)
