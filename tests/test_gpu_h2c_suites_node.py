"""RFC 9380 for secp256k1 and ed25519 through the N-API shim (addon/noble_gpu.js secp256k1_hasher, ed25519_hasher,
secp256k1HashToCurveBatch, secp256k1EncodeToCurveBatch, ed25519HashToCurveBatch, ed25519EncodeToCurveBatch, hashToScalarBatch):
addon/h2c_suites_test.js replays the listed rows of tests/golden/h2c_suites_kat.json and compares the points, the scalars and the
reference's messages."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "addon")

pytestmark = pytest.mark.gpu


def test_h2c_suites_through_the_shim():
    if not shutil.which("node") or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / N-API headers not available")
    if not os.path.exists(os.path.join(ADDON, "noble_gpu.node")):
        subprocess.check_call(["make", "-C", ADDON], stdout=subprocess.DEVNULL)
    r = subprocess.run(["node", os.path.join(ADDON, "h2c_suites_test.js")], cwd=ADDON, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "h2c suites OK" in r.stdout
