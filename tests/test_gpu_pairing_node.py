"""bls12-381 pairings through the N-API shim (addon/noble_gpu.js pairingBatch, blsVerifyBatch): addon/pairing_test.js replays the
reference's answers of tests/golden/bls12_381_pairing_kat.json on inputs rebuilt here by tests/pairing_helpers.py."""
import json
import os
import shutil
import subprocess

import pytest

import pairing_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "addon")

pytestmark = pytest.mark.gpu


def test_pairing_through_the_shim(tmp_path):
    if not shutil.which("node") or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / N-API headers not available")
    if not os.path.exists(os.path.join(ADDON, "noble_gpu.node")):
        subprocess.check_call(["make", "-C", ADDON], stdout=subprocess.DEVNULL)
    row = lambda p, q: [H.g1_wire(p).hex(), H.g2_wire(q).hex()]  # noqa: E731
    inp = {"vectors": [row(H.g1_mul(i + 1), H.g2_mul(i + 1)) for i in range(8)],
           "batch": [[row(H.g1_mul(a), H.g2_mul(b)) for a, b in H.seeded_batch(j)] for j in range(8)],
           "verify": {k: v for k, v in H.verify_rows().items() if not k.endswith("_batch")},
           "torsion_g1": H.g1_wire(H.torsion_points()[0]).hex()}
    f = tmp_path / "pairing_in.json"
    f.write_text(json.dumps(inp))
    r = subprocess.run(["node", os.path.join(ADDON, "pairing_test.js"), str(f)], cwd=ADDON, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "pairing OK" in r.stdout
