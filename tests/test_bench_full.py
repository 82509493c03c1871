"""`bench.py` without `--full` runs only the timed steps of each workload and the checks of what they computed; the legs beside them
(host-pointer, in-flight, window-share and resident-set timings, power_state, the host information of the CPU baseline) run with
`--full` alone, and neither form changes what the timed steps compute."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY_MSM = ("end_to_end", "pipelined", "window_share", "resident_subgroup_set", "power_state")


def _run(out_dir, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--log2n", "12",
                        "--out", str(out_dir / "full.json"), "--dump-outputs", str(out_dir / "dump")] + list(flags),
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0]), json.loads((out_dir / "full.json").read_text().strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_plain_run_leaves_the_full_legs_out(tmp_path):
    a, b = tmp_path / "plain", tmp_path / "full"
    line_p, plain = _run(a)
    line_f, full = _run(b, "--full", "--no-cpu-baseline", "--no-live-pmc")
    for line in (line_p, line_f):
        assert line["metric"] == "secp256k1_scalar_mults_per_sec" and line["steps"] == 2 and line["warmup"] == 1
        assert line["value"] > 0 and line["ms_per_step"] > 0
    # the plain run: the timed steps of every workload, nothing beside them
    assert len(plain["step_times"]["event_ms"]["list"]) == 2
    for key in ("end_to_end", "power_state", "host", "cpu_baseline"):
        assert key not in plain, key
    assert set(plain["extra"]) == {"msm_g1", "msm_g2", "ed25519_verify", "ntt_fr"}
    for key in ("msm_g1", "msm_g2"):
        assert len(plain["extra"][key]["step_times"]["event_ms"]["list"]) == 2
        for k in FULL_ONLY_MSM:
            assert k not in plain["extra"][key], (key, k)
    assert "power_state" not in plain["extra"]["ed25519_verify"] and "cpu_baseline" not in plain["extra"]["ntt_fr"]
    assert plain["pmc"].startswith("committed profile")
    # --full: the legs are back
    assert "end_to_end" in full and "host" in full
    for key in ("msm_g1", "msm_g2"):
        for k in ("end_to_end", "pipelined", "window_share", "resident_subgroup_set"):
            assert k in full["extra"][key], (key, k)
    # and the timed steps computed the same in both
    names = sorted(os.listdir(str(a / "dump")))
    assert names == sorted(os.listdir(str(b / "dump"))) and len(names) == 9
    for name in names:
        assert np.array_equal(np.load(str(a / "dump" / name)), np.load(str(b / "dump" / name))), name
