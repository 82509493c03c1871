"""The reference's own bn254.G1.Point (src/bn254.ts, js_hooked/ of oracle/_ref/refjs.bundle) through the shim: registered as
gpu.CURVE.BN254_G1, installed as the backend of the reference's `pippenger`, compared with the reference's own loop
(addon/bn254_redirect_test.mjs)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "addon")

pytestmark = pytest.mark.gpu


def test_reference_bn254_points_through_the_redirect():
    sys.path.insert(0, ROOT)
    from oracle import refjs
    if not shutil.which("node") or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / N-API headers not available")
    if not refjs.available() or refjs.hooked_dir() is None:
        pytest.skip("oracle/_ref/refjs.bundle (with js_hooked/) not built - needs /root/reference at build time")
    if not os.path.exists(os.path.join(ADDON, "noble_gpu.node")):
        subprocess.check_call(["make", "-C", ADDON], stdout=subprocess.DEVNULL)
    r = subprocess.run(["node", os.path.join(ADDON, "bn254_redirect_test.mjs"), refjs.hooked_dir()], cwd=ADDON, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bn254 redirect OK" in r.stdout
