"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as float32 .npy files within 64 MB, the same on
every run with the same arguments (so that two builds can be compared output for output); `--steps` sets the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n = 1 << 20
    rows = bench.OutputDump.rows(n, 256)
    assert np.array_equal(rows, bench.OutputDump.rows(n, 256))                     # the same rows on every run
    assert len(rows) <= bench.DUMP_ROWS + 3 and rows[0] == 0 and rows[2] == 2 and rows[-1] < n
    assert np.all(np.diff(rows) > 0)
    assert np.array_equal(bench.OutputDump.rows(1000, 256), np.arange(1000))        # short outputs are written whole
    assert np.array_equal(bench.OutputDump.rows(n, 4), np.arange(n))                # so are long ones that fit the per-array budget
    d = bench.OutputDump(str(tmp_path / "d"))
    t = torch.randint(0, 256, (n, 64), dtype=torch.uint8)
    d.add_rows("pts", t)
    d.add("one", [True])
    d.write()
    got = np.load(str(tmp_path / "d" / "pts.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, t.numpy()[rows].astype(np.float32))
    assert np.load(str(tmp_path / "d" / "one.npy")).tolist() == [1.0]
    big = bench.OutputDump(str(tmp_path / "e"))
    big.add("x", np.zeros((bench.DUMP_MAX_BYTES // 4 + 1,), np.uint8))
    with pytest.raises(AssertionError, match="budget"):
        big.write()


def _run(out_dir, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--log2n", "12",
                        "--quick-verify", "--no-cpu-baseline", "--no-live-pmc", "--out", str(out_dir / "full.json"),
                        "--dump-outputs", str(out_dir / "dump")], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_bench_dump_outputs_are_reproducible(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    la, lb = _run(a, 3), _run(b, 2)
    assert la["steps"] == 3 and lb["steps"] == 2 and la["ms_per_step"] > 0 and lb["ms_per_step"] > 0
    full = json.loads((a / "full.json").read_text().strip().splitlines()[-1])
    assert len(full["step_times"]["event_ms"]["list"]) == 3                      # exactly K timed steps
    names = sorted(os.listdir(str(a / "dump")))
    assert names == sorted(os.listdir(str(b / "dump")))
    for want in ("secp256k1_points", "secp256k1_infinity", "msm_g1_point", "msm_g1_infinity", "msm_g2_point", "msm_g2_infinity",
                 "ed25519_valid", "ed25519_valid_prehashed", "ntt_fr"):
        assert want + ".npy" in names, names
    total = 0
    for name in names:
        x, y = np.load(str(a / "dump" / name)), np.load(str(b / "dump" / name))
        assert x.dtype in (np.float32, np.float64) and x.dtype == y.dtype
        assert np.array_equal(x, y), name
        total += x.nbytes
    assert total <= 64 << 20
    pts = np.load(str(a / "dump" / "secp256k1_points.npy"))
    assert pts.shape == (1 << 12, 64) and pts.min() >= 0 and pts.max() <= 255
    assert np.load(str(a / "dump" / "secp256k1_infinity.npy")).tolist()[:2] == [1.0, 0.0]    # k = 0 at row 0, k = 1 at row 1
    assert np.load(str(a / "dump" / "msm_g1_point.npy")).shape == (96,)
    assert np.load(str(a / "dump" / "msm_g2_point.npy")).shape == (192,)
