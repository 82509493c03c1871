"""RFC 9380 for edwards448 and decaf448 through the N-API shim (addon/noble_gpu.js ed448_hasher, ed448HashToCurveBatch,
ed448EncodeToCurveBatch, decaf448HashToCurveBatch, decaf448HashToScalarBatch): addon/h2c448_test.js replays the listed rows of
tests/golden/h2c448_kat.json and compares the points, the encodings, the scalars and the reference's messages."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "addon")

pytestmark = pytest.mark.gpu


def test_h2c448_through_the_shim():
    if not shutil.which("node") or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / N-API headers not available")
    if not os.path.exists(os.path.join(ADDON, "noble_gpu.node")):
        subprocess.check_call(["make", "-C", ADDON], stdout=subprocess.DEVNULL)
    r = subprocess.run(["node", os.path.join(ADDON, "h2c448_test.js")], cwd=ADDON, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "h2c448 OK" in r.stdout
