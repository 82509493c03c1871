"""Ed448 signing and verification from messages through the N-API shim (addon/noble_gpu.js ed448GetPublicKeyBatch, ed448SignBatch,
ed448VerifyBatch with deviceHash and the single-item helpers): addon/ed448_sign_test.js replays the reference's own answers of
tests/golden/ed448_sign_kat.json and compares the messages."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "addon")

pytestmark = pytest.mark.gpu


def test_ed448_sign_through_the_shim():
    if not shutil.which("node") or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / N-API headers not available")
    if not os.path.exists(os.path.join(ADDON, "noble_gpu.node")):
        subprocess.check_call(["make", "-C", ADDON], stdout=subprocess.DEVNULL)
    r = subprocess.run(["node", os.path.join(ADDON, "ed448_sign_test.js")], cwd=ADDON, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ed448 sign OK" in r.stdout
