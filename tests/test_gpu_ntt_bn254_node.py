"""The bn254 scalar-field transform through the N-API shim (addon/noble_gpu.js fftFr with opts.field = 'bn254'):
addon/fft_bn254_test.js - the reference's bn254 roots(3) / brp(3) known answers as the transform of the delta at 1, round
trips in two orderings, "outside of range" for a value >= r."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "addon")

pytestmark = pytest.mark.gpu


def test_bn254_fft_through_the_shim():
    if not shutil.which("node") or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / N-API headers not available")
    if not os.path.exists(os.path.join(ADDON, "noble_gpu.node")):
        subprocess.check_call(["make", "-C", ADDON], stdout=subprocess.DEVNULL)
    r = subprocess.run(["node", os.path.join(ADDON, "fft_bn254_test.js")], cwd=ADDON, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bn254 fft OK" in r.stdout
