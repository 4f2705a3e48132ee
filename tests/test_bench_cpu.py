"""bench.py's command line on a box without a GPU: a plain run times exactly --steps steps and measures nothing beyond the headline;
the rest is behind --full; --dump-outputs needs the real workload."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_plain_run_defaults():
    a = _bench().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.windows == 1
    assert not a.full and a.dump_outputs is None
    a = _bench().parse_args(["--full", "--no-cpu", "--dump-outputs", "d"])
    assert a.full and a.no_cpu and a.dump_outputs == "d"


def test_timed_windows_launch_exactly_steps():
    calls = []
    out = _bench().timed_windows(lambda: calls.append(1), 7, 1, lambda: None, 1, "cpu", use_events=False)
    assert len(calls) == 7 and len(out) == 1


def test_stub_run_line_has_the_headline_keys():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--stub-workload", "--steps", "4", "--warmup", "1",
                        "--preroll-ms", "1"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res, key
    assert res["steps"] == 4 and 0.9 < res["ms_per_step"] < 20.0


def test_dump_outputs_refuses_the_stub(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub-workload", "--steps", "1", "--dump-outputs", str(tmp_path / "o")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr
    assert not (tmp_path / "o").exists()


@pytest.mark.parametrize("rows", [512, 5000])
def test_dump_outputs_writes_float32_within_64mb(tmp_path, rows):
    import numpy as np
    import torch
    bench = _bench()
    B, S, H, D = 2, 1000, 3, 16
    out = torch.randn(B, S, H, D).bfloat16()
    lse = torch.randn(B, H, S)
    bench.dump_outputs(str(tmp_path), out, lse, rows=rows)
    o, l = np.load(tmp_path / "out.npy"), np.load(tmp_path / "lse.npy")
    assert o.dtype == np.float32 and l.dtype == np.float32
    assert o.shape == (B, min(rows, S), H, D) and l.shape == (B, H, S)
    assert np.array_equal(l, lse.numpy())
    idx = torch.randperm(S, generator=torch.Generator().manual_seed(0))[:min(rows, S)].sort().values
    assert np.array_equal(o, out[:, idx].float().numpy())
