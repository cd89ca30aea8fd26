"""The transform over point sets through the N-API addon and the JS facade: the exports (no GPU), and js/test-points-ntt.js
(`-m gpu`)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
NAMES = ("pointsNtt",)


def _addon():
    if NODE is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node_api.h not present")
    from conftest import build_if_missing

    build_if_missing("all", "montgomery_amd/libmsm_hip.so")
    build_if_missing("napi", "montgomery_amd/msm_hip.node")


def test_addon_and_facade_export_the_points_ntt_entry():
    _addon()
    out = subprocess.run([NODE, "-e", "const m=require('./js/montgomery-hip.js');console.log(Object.keys(m.hip).sort().join(','))"],
                         cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    names = out.stdout.strip().split(",")
    for n in NAMES:
        assert n in names
    js = open(os.path.join(ROOT, "js", "montgomery-hip.js")).read()
    dts = open(os.path.join(ROOT, "js", "montgomery-hip.d.ts")).read()
    for n in NAMES:
        assert f"{n}(" in js and f"{n}(" in dts, n


@pytest.mark.gpu
def test_js_points_ntt_equals_the_bigint_transform():
    _addon()
    out = subprocess.run([NODE, "js/test-points-ntt.js"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
