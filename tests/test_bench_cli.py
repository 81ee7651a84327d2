"""bench.py's command line: a plain run is the timed steps and the result
line alone (every other leg is behind --full), and --dump-outputs writes what
the last timed step's sv_ed25519_verify_device call returned.

The dump layout is checked on the CPU with hand-made verdicts; one small plain
run on the GPU (4099 signatures: a partial last bitmap word) checks the line's
keys, the step count and the dumped arrays.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("host_api", "in_process_multi_gpu", "latency_1k", "latency_1k_cold_keys", "cpu_baseline", "config1",
             "config3", "config4_integrated", "config5")


def test_dump_layout(tmp_path):
    torch = pytest.importorskip("torch")
    import bench
    n = 130
    verdict = torch.ones(n, dtype=torch.uint8)
    verdict[5] = 0
    bitmap = torch.tensor([-1, ~(1 << 3), 3], dtype=torch.int64)
    bench.dump_outputs(str(tmp_path / "d"), verdict, bitmap, n, 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == ["bitmap_bits.npy", "verdict.npy"]
    v = np.load(tmp_path / "d" / "verdict.npy")
    b = np.load(tmp_path / "d" / "bitmap_bits.npy")
    assert v.dtype == np.float32 and b.dtype == np.float32 and v.shape == b.shape == (n,)
    assert np.array_equal(v, verdict.numpy())
    want = np.ones(n, np.float32)
    want[64 + 3] = 0  # bit (i % 64) of word i / 64
    assert np.array_equal(b, want)
    # N > 1: one pair of files per rank
    bench.dump_outputs(str(tmp_path / "e"), verdict, bitmap, n, 1, 2)
    assert sorted(os.listdir(tmp_path / "e")) == ["bitmap_bits_rank1.npy", "verdict_rank1.npy"]


@pytest.mark.gpu
def test_plain_run_dumps_and_skips_full_legs(tmp_path):
    n, steps = 4099, 2
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--batch", str(n), "--dump-outputs", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == steps and line["kernel"]["launches"] == steps
    assert line["verdicts_ok"] is True
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(n * 1e3 / line["ms_per_step"], rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]
    v = np.load(tmp_path / "verdict.npy")
    b = np.load(tmp_path / "bitmap_bits.npy")
    assert v.dtype == np.float32 and b.dtype == np.float32 and v.shape == b.shape == (n,)
    assert (v == 1).all() and (b == 1).all()  # every signature of the bench dataset is valid
