"""FP8 forward against the bf16 paths a user has, in one process (profiles/fwd_fp8.txt).

    python tools/fp8_fwd_bench.py [--steps 30] [--warmup 5] [--quick]

Per shape, three timings of the same attention on the same (seeded, N(0,1)) data:
  fp8        flash_attn_amd backend fwd_fp8 on float8_e4m3fn q / k / v with (B, Hk) descales (C ABI fa_fwd_fp8);
  bf16       the default bf16 forward (fa_fwd) on the dequantised tensors;
  deq+bf16   what a caller with an fp8 model runs today: dequantise q / k / v in torch, then the bf16 forward.
Timing follows bench.py: an untimed clock ramp, W warm-up launches, then K launches between two HIP events.  FLOPs follow bench.py's
convention on the visible (query, key) pairs, 4 * B * H * D * pairs.  Fractions of peak use 5.0 PFLOP/s (fp8, dense) and 2.5 (bf16)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flash-attention_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench import time_kernel  # noqa: E402
from oracle.attention_oracle import attention_flops  # noqa: E402

FP8_PEAK, BF16_PEAK = 5000.0, 2500.0   # TFLOP/s, dense (MI355X_MICROARCH.md)

# (name, B, Sq, H, Hk, D, causal, window)
SHAPES = [
    ("config 3: B4 H32 S4096 D128 causal", 4, 4096, 32, 32, 128, True, (-1, -1)),
    ("D128 causal S1k (16k tokens)", 16, 1024, 16, 16, 128, True, (-1, -1)),
    ("D128 causal S4k (16k tokens)", 4, 4096, 16, 16, 128, True, (-1, -1)),
    ("D128 causal S16k (16k tokens)", 1, 16384, 16, 16, 128, True, (-1, -1)),
    ("D128 no mask S1k (16k tokens)", 16, 1024, 16, 16, 128, False, (-1, -1)),
    ("D128 no mask S4k (16k tokens)", 4, 4096, 16, 16, 128, False, (-1, -1)),
    ("D128 no mask S16k (16k tokens)", 1, 16384, 16, 16, 128, False, (-1, -1)),
    ("D64 no mask S4k (16k tokens)", 4, 4096, 32, 32, 64, False, (-1, -1)),
    ("config 5: B2 S8192 H32/8 D128 causal window 1024", 2, 8192, 32, 8, 128, True, (1024, 0)),
]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="config 3 only")
    a = ap.parse_args(argv)
    from flash_attn_amd import backend as be
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    rows = []
    for name, B, S, H, Hk, D, causal, win in SHAPES[:1] if a.quick else SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        q8 = torch.randn(B, S, H, D, device=dev, generator=g).to(torch.float8_e4m3fn)
        k8 = torch.randn(B, S, Hk, D, device=dev, generator=g).to(torch.float8_e4m3fn)
        v8 = torch.randn(B, S, Hk, D, device=dev, generator=g).to(torch.float8_e4m3fn)
        qd, kd, vd = (torch.rand(B, Hk, device=dev, generator=g) + 0.5 for _ in range(3))
        sc = D ** -0.5

        def deq(x, d):   # the caller's route today (not the product path): dequantise in torch
            return (x.to(torch.float32) * d.repeat_interleave(x.shape[2] // Hk, dim=1)[:, None, :, None]).to(torch.bfloat16)

        qb, kb, vb = deq(q8, qd), deq(k8, kd), deq(v8, vd)
        fp8 = lambda: be.fwd_fp8(q8, k8, v8, None, qd, kd, vd, sc, causal, win[0], win[1])
        bf16 = lambda: be.fwd(qb, kb, vb, None, None, 0.0, sc, causal, win[0], win[1], 0.0, False, None)
        dq_bf16 = lambda: be.fwd(deq(q8, qd), deq(k8, kd), deq(v8, vd), None, None, 0.0, sc, causal, win[0], win[1], 0.0, False, None)
        fl = attention_flops(B, H, S, S, D, causal, win)
        row = {"shape": name}
        for key, fn in (("fp8", fp8), ("bf16", bf16), ("deq+bf16", dq_bf16)):
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.3:   # clock ramp
                fn()
            sync()
            _, ms = time_kernel(fn, a.steps, a.warmup, sync)
            row[key + "_ms"] = round(ms, 4)
            row[key + "_tflops"] = round(fl / ms / 1e9, 1)
            if key == "fp8":
                row["fp8_kernel"] = be.last_schedule()["name"]
        row["fp8_of_peak"] = round(row["fp8_tflops"] / FP8_PEAK, 3)
        row["bf16_of_peak"] = round(row["bf16_tflops"] / BF16_PEAK, 3)
        row["fp8_vs_deq+bf16"] = round(row["deq+bf16_ms"] / row["fp8_ms"], 3)
        row["fp8_vs_bf16"] = round(row["bf16_ms"] / row["fp8_ms"], 3)
        row["max|fp8-bf16| out"] = round(float((fp8()[0].float() - bf16()[0].float()).abs().max()), 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del q8, k8, v8, qb, kb, vb
        torch.cuda.empty_cache()
    return rows


if __name__ == "__main__":
    main()
