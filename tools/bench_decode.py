"""Decode (KV-cache, one query token) bandwidth: bytes of K and V actually attended / time, vs the HBM roofline.
usage: bench_decode.py [num_splits ...]   (0 = heuristic, 1 = unsplit)
       bench_decode.py --fp8 [--reps 30] [--kernels]
--fp8 (profiles/fwd_kvcache_fp8.txt): every shape twice in one process -- the bf16 cache through fwd_kvcache, and the same values quantised to e4m3
(per-(batch, kv head) scales) through fwd_kvcache_fp8 -- heuristic splits, a warm-up, then the median of --reps individually timed calls with the
spread (min .. max) of the repeats.  --kernels runs three shapes a few times and nothing else: the body of a `rocprofv3 --kernel-trace --stats` run."""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention_amd"))
import torch
from flash_attn_amd import backend as be

HBM_PEAK = 8000.0  # GB/s
SHAPES = ((1, 8192), (1, 32768), (1, 131072), (8, 8192), (8, 32768), (64, 4096), (64, 16384), (256, 4096))
GATED = {(8, 32768), (64, 4096), (64, 16384), (256, 4096)}   # bandwidth-bound: B >= 64, or B = 8 with Sk = 32k
H, Hk, D = 32, 8, 128


def t_ms(fn, reps=20):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def each_ms(fn, reps):
    """reps individually timed calls -> sorted list of ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) for e0, e1 in ev)


def make(B, S):
    """bf16 q / caches and their e4m3 quantisation: scale = amax / 448 per (batch, kv head), as a caller of the fp8 prefill would choose it"""
    q = torch.randn(B, 1, H, D, device="cuda", dtype=torch.bfloat16)
    kc = torch.randn(B, S, Hk, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")

    def quant(x, heads_per):
        xs = x.float().reshape(B, x.shape[1], Hk, heads_per * D)
        sc = (xs.abs().amax(dim=(1, 3)) / 448.0).clamp_min(1e-12)   # (B, Hk)
        return (xs / sc[:, None, :, None]).reshape(x.shape).to(torch.float8_e4m3fn), sc.contiguous()

    (q8, qd), (k8, kd), (v8, vd) = quant(q, H // Hk), quant(kc, 1), quant(vc, 1)
    return (q, kc, vc), (q8, k8, v8, qd, kd, vd), lens


def main_fp8(reps, kernels_only):
    shapes = ((1, 131072), (8, 32768), (64, 16384)) if kernels_only else SHAPES
    print(f"# decode, H={H}/{Hk} D={D}, one query token, contiguous cache, cache_seqlens = Sk, heuristic splits; median of {reps} timed calls [min .. max]")
    for B, S in shapes:
        (q, kc, vc), (q8, k8, v8, qd, kd, vd), lens = make(B, S)
        f16 = lambda: be.fwd_kvcache(q, kc, vc, None, None, lens, None, None, None, None, None, None, None, D ** -0.5, False, -1, -1, 0.0, True, 0)
        f8 = lambda: be.fwd_kvcache_fp8(q8, k8, v8, None, None, lens, None, None, None, qd, kd, vd, D ** -0.5, False, -1, -1, 0)
        if kernels_only:
            for f in (f16, f8):
                for _ in range(10):
                    f()
            torch.cuda.synchronize()
            continue
        res = {}
        for name, f, bytes_per in (("bf16", f16, 2), ("fp8", f8, 1)):
            for _ in range(5):
                f()
            t = each_ms(f, reps)
            s = be.last_schedule()
            res[name] = (statistics.median(t), t[0], t[-1], 2 * B * S * Hk * D * bytes_per / 1e9, s["fwd_splits"], s["name"])
        err = float((f8()[0].float() - f16()[0].float()).abs().max())
        line = f"decode B={B:3d} Sk={S:6d}{' *' if (B, S) in GATED else '  '}"
        for name in ("bf16", "fp8"):
            med, lo, hi, gb, ns, _ = res[name]
            line += f" | {name} {med * 1e3:7.1f} us [{lo * 1e3:7.1f} .. {hi * 1e3:7.1f}] {gb / med * 1e3:6.0f} GB/s splits={ns:2d}"
        b, f = res["bf16"], res["fp8"]
        line += f" | bf16/fp8 time = {b[0] / f[0]:.3f}  (bf16 spread {(b[2] - b[1]) * 1e3:.1f} us, gain {(b[0] - f[0]) * 1e3:.1f} us)  max|fp8-bf16| = {err:.3f}"
        print(line, flush=True)
        del q, kc, vc, q8, k8, v8
        torch.cuda.empty_cache()
    if not kernels_only:
        print(f"# (* = the bandwidth-bound shapes; GB/s = bytes of K and V actually read / time; fp8 kernel: {res['fp8'][5]})")


def main():
    if "--fp8" in sys.argv:
        reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
        return main_fp8(max(20, reps), "--kernels" in sys.argv)
    splits = [int(x) for x in sys.argv[1:]] or [1, 0]
    for B, S in SHAPES:
        q = torch.randn(B, 1, H, D, device="cuda", dtype=torch.bfloat16)
        kc = torch.randn(B, S, Hk, D, device="cuda", dtype=torch.bfloat16)
        vc = torch.randn_like(kc)
        lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
        gb = 2 * B * S * Hk * D * 2 / 1e9
        line = f"decode B={B:3d} Sk={S:6d} H={H}/{Hk} D={D} ({gb * 1e3:7.1f} MB of K,V):"
        for ns in splits:
            f = lambda: be.fwd_kvcache(q, kc, vc, None, None, lens, None, None, None, None, None, None, None, D ** -0.5, False, -1, -1, 0.0, True, ns)
            f()
            ms = statistics.median([t_ms(f) for _ in range(5)])
            line += f"  [splits={ns}] {ms * 1e3:8.1f} us {gb / ms * 1e3:7.0f} GB/s ({gb / ms * 1e3 / HBM_PEAK * 100:4.1f}% of HBM peak)"
        print(line, flush=True)


if __name__ == "__main__":
    main()
