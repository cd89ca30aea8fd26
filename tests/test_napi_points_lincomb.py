"""Point-set linear combinations through the N-API addon and the JS facade: the exports (no GPU), and
js/test-points-lincomb.js (`-m gpu`)."""
import pytest

from napi_support import assert_exports, run_js

NAMES = ("pointsLincomb", "pointsetSize")


def test_addon_and_facade_export_the_lincomb_entries():
    assert_exports(NAMES, facade=NAMES + ("foldPoints",))


@pytest.mark.gpu
def test_js_points_lincomb_equals_msm_over_the_sources():
    run_js("test-points-lincomb.js", 600)
