"""bench.py on the GPU: a plain run prints the headline line and nothing beyond it; --dump-outputs writes what the last timed step returned
(float32, within 64 MB), the same files from run to run, and those files are the attention of the seeded inputs (checked on a sample of
(batch, head) units against PyTorch fp32)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(d):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--preroll-ms", "50",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(tmp_path):
    res = _run(tmp_path / "a")
    assert res["metric"] == "attention_fwd_tflops" and res["unit"] == "TFLOP/s" and res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["steps"] == 3 and res["windows"]["n"] == 1 and res["value"] > 0 and res["ms_per_step"] > 0
    for key in ("fwd_bwd", "sweep_d128", "configs", "parity_max_abs_err", "cpu_baseline", "extras_file"):
        assert key not in res, key                           # --full only
    assert res["roofline"]["traffic"] is None
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["lse.npy", "out.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 2 ** 20
    out, lse = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "a" / "lse.npy")
    B, S, H, D = 4, 4096, 32, 128
    assert out.dtype == np.float32 and lse.dtype == np.float32
    assert out.shape == (B, 512, H, D) and lse.shape == (B, H, S)
    assert np.isfinite(out).all() and np.isfinite(lse).all()

    _run(tmp_path / "b")                                     # same arguments: same inputs, same bits
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f

    # the inputs bench.py draws (rank 0), and the rows its sample keeps
    torch.manual_seed(0)
    q = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16)
    idx = torch.randperm(S, generator=torch.Generator().manual_seed(0))[:512].sort().values.cuda()
    causal = torch.arange(S, device="cuda")[None, :] > idx[:, None]
    for b, h in ((0, 0), (1, 17), (3, 31)):
        s = (q[b, idx, h].float() @ k[b, :, h].float().T) * D ** -0.5
        s = s.masked_fill(causal, float("-inf"))
        o_ref = (torch.softmax(s, dim=-1) @ v[b, :, h].float()).cpu().numpy()
        l_ref = torch.logsumexp(s, dim=-1).cpu().numpy()
        assert np.abs(out[b, :, h] - o_ref).max() < 2e-2, (b, h)
        assert np.abs(lse[b, h, idx.cpu().numpy()] - l_ref).max() < 8e-3, (b, h)    # the 64-rows-per-wave kernel's LSE bound (test_baseline_configs_gpu)
