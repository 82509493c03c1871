"""The ristretto255 OPRF through the N-API shim (addon/noble_gpu.js ristretto255_oprf: oprf, voprf, poprf(info) with their batch
forms): addon/oprf_test.js replays the reference's own answers of tests/golden/ristretto255_oprf_kat.json with the recorded rng
bytes and compares the messages."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "addon")

pytestmark = pytest.mark.gpu


def test_oprf_through_the_shim():
    if not shutil.which("node") or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / N-API headers not available")
    if not os.path.exists(os.path.join(ADDON, "noble_gpu.node")):
        subprocess.check_call(["make", "-C", ADDON], stdout=subprocess.DEVNULL)
    r = subprocess.run(["node", os.path.join(ADDON, "oprf_test.js")], cwd=ADDON, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ristretto255 OPRF OK" in r.stdout
