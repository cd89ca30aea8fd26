"""What the test_napi_*.py files share: the addon build (or the skip without node), the export checks and the runner of
the js/test-*.js scripts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


def require_addon():
    """Skips without node or its N-API header; otherwise the library and the addon are there when it returns."""
    if NODE is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node_api.h not present")
    from conftest import build_if_missing

    build_if_missing("all", "montgomery_amd/libmsm_hip.so")
    build_if_missing("napi", "montgomery_amd/msm_hip.node")
    return os.path.join(ROOT, "montgomery_amd", "msm_hip.node")


def exported_names():
    """The keys of the addon as the facade loads it (needs no GPU)."""
    out = subprocess.run([NODE, "-e", "const m=require('./js/montgomery-hip.js');console.log(Object.keys(m.hip).sort().join(','))"],
                         cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return out.stdout.strip().split(",")


def assert_exports(names, facade=None, hip_calls=()):
    """`names` are keys of the addon; `facade` (default: the same names) are methods of both js/montgomery-hip.js and its
    .d.ts; `hip_calls` are addon entries the facade itself calls."""
    require_addon()
    exported = exported_names()
    for n in names:
        assert n in exported, n
    js = open(os.path.join(ROOT, "js", "montgomery-hip.js")).read()
    dts = open(os.path.join(ROOT, "js", "montgomery-hip.d.ts")).read()
    for n in names if facade is None else facade:
        assert f"{n}(" in js and f"{n}(" in dts, n
    for n in hip_calls:
        assert f"hip.{n}(" in js, n


def run_js(script, timeout, *args):
    """`node js/<script> args...` from the repository root: exit code 0 and the script's closing "ALL OK"."""
    require_addon()
    out = subprocess.run([NODE, f"js/{script}", *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
