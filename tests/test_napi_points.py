"""pointsFromBytes(..., {compressed, validate}) of the JS facade (js/test-points-compressed.js).  `-m gpu`."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.gpu
def test_js_compressed_points(tmp_path):
    if NODE is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node_api.h not present")
    from conftest import build_if_missing
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmContext

    build_if_missing("all", "montgomery_amd/libmsm_hip.so")
    build_if_missing("napi", "montgomery_amd/msm_hip.node")
    n = 1 << 14
    for name, cid in (("bls377", _lib.CURVE_BLS12_377_G1), ("bls381", _lib.CURVE_BLS12_381_G1), ("ed377", _lib.CURVE_ED_ON_BLS12_377)):
        ctx = MsmContext(cid)
        try:
            ctx.generate_points(n, seed=77)
            (tmp_path / f"{name}.raw").write_bytes(ctx.get_points(0, n))
            (tmp_path / f"{name}.cmp").write_bytes(ctx.get_points(0, n, compressed=True))
        finally:
            ctx.close()
    out = subprocess.run([NODE, "js/test-points-compressed.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
