"""pointsFromBytes(..., {compressed, validate}) of the JS facade (js/test-points-compressed.js).  `-m gpu`."""
import pytest

from napi_support import require_addon, run_js


@pytest.mark.gpu
def test_js_compressed_points(tmp_path):
    require_addon()
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmContext

    n = 1 << 14
    for name, cid in (("bls377", _lib.CURVE_BLS12_377_G1), ("bls381", _lib.CURVE_BLS12_381_G1), ("ed377", _lib.CURVE_ED_ON_BLS12_377)):
        ctx = MsmContext(cid)
        try:
            ctx.generate_points(n, seed=77)
            (tmp_path / f"{name}.raw").write_bytes(ctx.get_points(0, n))
            (tmp_path / f"{name}.cmp").write_bytes(ctx.get_points(0, n, compressed=True))
        finally:
            ctx.close()
    run_js("test-points-compressed.js", 600, str(tmp_path))
