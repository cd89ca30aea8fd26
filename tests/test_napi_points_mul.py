"""Per-row scalar multiplication through the N-API addon and the JS facade: the exports (no GPU), and js/test-points-mul.js
(`-m gpu`)."""
import pytest

from napi_support import assert_exports, run_js

NAMES = ("pointsMul", "pointsMulBase")


def test_addon_and_facade_export_the_points_mul_entries():
    assert_exports(NAMES)


@pytest.mark.gpu
def test_js_points_mul_equals_msm_over_the_sources():
    run_js("test-points-mul.js", 600)
