"""Absorbed MLA decode (q / k 576, v / o 512, v_cache = k_cache[..., :512]; fa_fwd_mla_kernel) against the route a user had before it existed: the
same attention composed from PyTorch bf16 matmul / fp32 softmax / matmul over the same cache (profiles/fwd_mla_decode.txt).

    python tools/mla_decode_ab.py [--windows 7] [--steps 10] [--out profiles/fwd_mla_decode.txt]

One process, one GPU.  bf16, Hk = 1, Sq = 1, H in {16, 128}, (B, Sk) in {(64, 4096), (8, 32768), (1, 131072)}, contiguous and paged (256-key pages,
shuffled).  Routes per shape:
  mla     flash_attn_with_kvcache(q, kv, kv[..., :512], cache_seqlens=Sk[, block_table]);
  torch   softmax(q . kv^T * scale) . kv[..., :512] with torch.matmul in bf16 and the softmax in fp32; for the paged cache the pages are gathered
          first (kv[block_table]), as a user without a paged kernel has to;
  d128    the existing bf16 head-dim-128 decode of this library at the same cache bytes: Hk = 9 KV heads of K and V (9 * 2 * 128 * 2 B = 4 x 1152 B
          per key) over Sk / 4 keys, H = 72 -- exactly B * Sk * 1152 bytes of cache.  Printed next to mla, no bar.
After an untimed clock ramp and a warm-up of every route, the routes ALTERNATE: each window times `steps` launches of one route between two device
events, W windows per route.  Reported: the median window, the spread (max - min) / median of the windows, cache bytes per second
(B * Sk * 1152 B per call) and TFLOP/s on 2 * rows * keys * (576 + 512).
Bar: mla is faster than torch at every shape by more than the larger of the two window spreads."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flash-attention_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

D, DV, PAGE = 576, 512, 256
SHAPES = [(64, 4096), (8, 32768), (1, 131072)]
HEADS = [16, 128]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)
    assert a.windows >= 5, "at least 5 windows per route"
    if not torch.cuda.is_available():
        raise SystemExit("mla_decode_ab.py measures on the GPU: no device found")
    from flash_attn_amd import backend as be
    from flash_attn_amd import flash_attn_with_kvcache
    dev = torch.device("cuda", 0)
    dt = torch.bfloat16
    sc = D ** -0.5
    sync = torch.cuda.synchronize
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/mla_decode_ab.py: bf16, Hk=1, Sq=1, D={D} Dv={DV}; {a.windows} windows x {a.steps} launches per route, routes alternating; "
             f"device {torch.cuda.get_device_name(0)}",
             "# cache GB/s = B * Sk * 1152 B per call; TFLOP/s = 2 * rows * keys * (576 + 512); d128 = the bf16 head-dim-128 decode at the same cache bytes"]
    results, all_ok = [], True
    for B, Sk in SHAPES:
        kv = torch.randn(B, Sk, 1, D, device=dev, dtype=dt, generator=g)
        per = Sk // PAGE
        order = torch.randperm(B * per, device=dev, generator=g).reshape(B, per)
        pages = torch.empty(B * per, PAGE, 1, D, device=dev, dtype=dt)
        pages[order.reshape(-1)] = kv.reshape(B * per, PAGE, 1, D)
        bt = order.to(torch.int32)
        lens = torch.full((B,), Sk, dtype=torch.int32, device=dev)
        # the head-dim-128 decode at the same cache bytes
        k128 = torch.randn(B, Sk // 4, 9, 128, device=dev, dtype=dt, generator=g)
        v128 = torch.randn(B, Sk // 4, 9, 128, device=dev, dtype=dt, generator=g)
        q128 = torch.randn(B, 1, 72, 128, device=dev, dtype=dt, generator=g)
        lens128 = torch.full((B,), Sk // 4, dtype=torch.int32, device=dev)
        assert k128.numel() * 2 * 2 == kv.numel() * 2
        for H in HEADS:
            q = torch.randn(B, 1, H, D, device=dev, dtype=dt, generator=g)

            def torch_route(cache):
                s = torch.matmul(q[:, 0], cache[:, :, 0].transpose(1, 2))                     # (B, H, Sk) bf16
                p = torch.softmax(s.float() * sc, dim=-1).to(dt)
                return torch.matmul(p, cache[:, :, 0, :DV])                                  # (B, H, 512)

            for kind in ("contig", "paged"):
                if kind == "contig":
                    mla = lambda: flash_attn_with_kvcache(q, kv, kv[..., :DV], cache_seqlens=lens)
                    ref = lambda: torch_route(kv)
                else:
                    mla = lambda: flash_attn_with_kvcache(q, pages, pages[..., :DV], cache_seqlens=lens, block_table=bt)
                    ref = lambda: torch_route(pages[order].reshape(B, Sk, 1, D))
                d128 = lambda: flash_attn_with_kvcache(q128, k128, v128, cache_seqlens=lens128)
                routes = {"mla": mla, "torch": ref, "d128": d128}
                o = mla()
                sched = be.last_schedule()
                assert sched["fwd_kernel"] == 7, sched
                err = float((o[:, 0].float() - ref().float()).abs().max())
                d128()
                sched128 = be.last_schedule()
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.5:   # clock ramp
                    mla()
                sync()
                for fn in routes.values():              # warm-up of every route
                    for _ in range(3):
                        fn()
                sync()
                ms = {n: [] for n in routes}
                for _ in range(a.windows):              # routes alternate
                    for n, fn in routes.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.steps):
                            fn()
                        e1.record()
                        sync()
                        ms[n].append(e0.elapsed_time(e1) / a.steps)
                nbytes = B * Sk * D * 2
                flops = 2.0 * B * H * Sk * (D + DV)
                row = {"B": B, "Sk": Sk, "H": H, "kind": kind, "splits": sched["fwd_splits"], "max_abs_diff_vs_torch": err}
                lines.append(f"B={B} Sk={Sk} H={H} {kind}: {sched['name']} splits={sched['fwd_splits']} pack={sched['fwd_pack']}; d128: {sched128['name']} "
                             f"splits={sched128['fwd_splits']} pack={sched128['fwd_pack']}; max |mla - torch| = {err:.3g}")
                for n, xs in ms.items():
                    med = statistics.median(xs)
                    spread = (max(xs) - min(xs)) / med
                    row[n] = {"median_ms": round(med, 4), "spread": round(spread, 4), "cache_GBps": round(nbytes / med / 1e6, 1),
                              "tflops": round(flops / med / 1e9, 2) if n != "d128" else None, "windows_ms": [round(x, 4) for x in xs]}
                    tf = f"{flops / med / 1e9:7.2f} TFLOP/s" if n != "d128" else " " * 15
                    lines.append(f"  {n:6s} median {med:8.4f} ms  spread {100 * spread:5.1f} %  cache {nbytes / med / 1e6:7.1f} GB/s  {tf}  windows {row[n]['windows_ms']}")
                margin = max(row["mla"]["spread"], row["torch"]["spread"])
                ok = row["mla"]["median_ms"] < row["torch"]["median_ms"] * (1.0 - margin)
                row["bar"] = ok
                all_ok = all_ok and ok
                lines.append(f"  bar (mla faster than torch by more than the larger spread {100 * margin:.1f} %): {'MET' if ok else 'MISSED'}: "
                             f"mla / torch time = {row['mla']['median_ms'] / row['torch']['median_ms']:.3f}; mla / d128 cache rate = "
                             f"{row['mla']['cache_GBps'] / row['d128']['cache_GBps']:.3f}")
                results.append(row)
        del kv, pages, k128, v128
    lines.append(f"bar at every shape: {'MET' if all_ok else 'MISSED'}")
    report = "\n".join(lines)
    print(report)
    print(json.dumps({"shapes": results, "bar": all_ok}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report + "\n")
    return results


if __name__ == "__main__":
    main()
