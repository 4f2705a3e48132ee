"""e4m3 quantisation: libfa_gfx950_quant.so against the PyTorch composition the project used before it (quant() of tools/bench_decode.py: fp32 copy, abs,
amax, divide, clamp, divide, cast) followed by the existing e4m3 fa_kvcache_append -- both in this process, alternating, on the same inputs.

Each side is timed two ways, after warm-up: EAGER (HIP events around a loop of --steps calls: what a Python caller pays, host launch cost included) and GRAPH
(the same loop captured in one HIP graph and replayed: the device-side cost, kernel boundaries included).  Medians of --reps windows, [min .. max].
bytes = what the algorithm has to move (two-pass dynamic: the input twice and the output once; one launch or static: input once, output once), shown as
bytes / graph time next to the 6.3 TB/s a streaming kernel achieves on this part.  Launches are counted with the profiler in a run of the loop body.

usage: python tools/bench_quant.py [--steps 20] [--reps 15] [--rows decode,prompt,config3] [--out profiles/quant_fp8.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention_amd"))
import torch  # noqa: E402

from flash_attn_amd import _cabi, kvcache_append_fp8, quantize_fp8  # noqa: E402

FP8 = torch.float8_e4m3fn
DEV = "cuda"
HBM_TBS = 6.3


def quant_dynamic(x, hk):
    """tools/bench_decode.py quant(): per-(batch entry, KV head) amax / 448."""
    B, S, H, D = x.shape
    xs = x.float().reshape(B, S, hk, (H // hk) * D)
    sc = (xs.abs().amax(dim=(1, 3)) / 448.0).clamp_min(1e-12)
    return (xs / sc[:, None, :, None]).reshape(x.shape).to(FP8), sc.contiguous()


def quant_static(x, sc):
    """The same composition with a given scale (the cache's): what a decode step did to the new token's k / v."""
    B, S, H, D = x.shape
    return (x.float() / sc[:, None, :, None]).clamp(-448.0, 448.0).to(FP8)


def byte_append(kc, vc, k8, v8, lens):
    lib = _cabi.load()
    ap = _cabi.FaKvAppendParams()
    ap.knew, ap.vnew, ap.kcache, ap.vcache = k8.data_ptr(), v8.data_ptr(), kc.data_ptr(), vc.data_ptr()
    for nm, t in (("knew", k8), ("vnew", v8), ("kcache", kc), ("vcache", vc)):
        setattr(ap, nm + "_batch_stride", t.stride(0)); setattr(ap, nm + "_row_stride", t.stride(1)); setattr(ap, nm + "_head_stride", t.stride(2))
    ap.seqlens_k = lens.data_ptr()
    ap.b, ap.seqlen_new, ap.h_k, ap.d, ap.dtype = k8.shape[0], k8.shape[1], k8.shape[2], k8.shape[3], _cabi.FA_DTYPE_FP8_E4M3
    _cabi.check(lib.fa_kvcache_append(C.byref(ap), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(); torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:   # no device tracer in this build: the table says so
        return None


def time_eager(fn, steps, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / steps)
    return out


def make_graph(fn, steps):
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(steps):
            fn()
    return g


def time_graph(g, steps, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / steps)
    return out


def fmt(ts):
    return f"{statistics.median(ts):9.1f} [{min(ts):8.1f} .. {max(ts):8.1f}]"


def rows(which):
    """(label, ours, parent, bytes ours has to move)"""
    torch.manual_seed(0)
    H, HK, D = 32, 8, 128
    if "decode" in which:
        for B in (1, 8, 64):
            q = torch.randn(B, 1, H, D, device=DEV, dtype=torch.bfloat16)
            k, v = torch.randn(B, 1, HK, D, device=DEV, dtype=torch.bfloat16), torch.randn(B, 1, HK, D, device=DEV, dtype=torch.bfloat16)
            kc, vc = torch.zeros(B, 4096, HK, D, dtype=torch.uint8, device=DEV).view(FP8), torch.zeros(B, 4096, HK, D, dtype=torch.uint8, device=DEV).view(FP8)
            lens = torch.full((B,), 1000, dtype=torch.int32, device=DEV)
            kd, vd = torch.rand(B, HK, device=DEV) + 0.5, torch.rand(B, HK, device=DEV) + 0.5

            def ours(q=q, k=k, v=v, kc=kc, vc=vc, lens=lens, kd=kd, vd=vd):
                quantize_fp8(q, num_heads_k=HK)
                kvcache_append_fp8(kc, vc, k, v, lens, kd, vd)

            def parent(q=q, k=k, v=v, kc=kc, vc=vc, lens=lens, kd=kd, vd=vd):
                quant_dynamic(q, HK)
                byte_append(kc, vc, quant_static(k, kd), quant_static(v, vd), lens)

            yield f"decode step B={B} (q 32/8 heads dynamic + 1-token k/v append)", ours, parent, 3 * (q.numel() + 2 * k.numel())
    if "prompt" in which:
        B, S = 4, 4096
        k, v = torch.randn(B, S, HK, D, device=DEV, dtype=torch.bfloat16), torch.randn(B, S, HK, D, device=DEV, dtype=torch.bfloat16)
        kc, vc = torch.zeros(B, S, HK, D, dtype=torch.uint8, device=DEV).view(FP8), torch.zeros(B, S, HK, D, dtype=torch.uint8, device=DEV).view(FP8)
        lens = torch.zeros(B, dtype=torch.int32, device=DEV)
        kd, vd = torch.rand(B, HK, device=DEV) + 0.5, torch.rand(B, HK, device=DEV) + 0.5

        def ours_dyn():
            (k8, _), (v8, _) = quantize_fp8(k=k, v=v, num_heads_k=HK)
            byte_append(kc, vc, k8, v8, lens)

        def parent_dyn():
            byte_append(kc, vc, quant_dynamic(k, HK)[0], quant_dynamic(v, HK)[0], lens)

        def ours_static():
            kvcache_append_fp8(kc, vc, k, v, lens, kd, vd)

        def parent_static():
            byte_append(kc, vc, quant_static(k, kd), quant_static(v, vd), lens)

        n = 2 * k.numel()
        yield "prompt K/V B=4 S=4096 Hk=8 into a cache, new (dynamic) scales", ours_dyn, parent_dyn, n * (2 * 2 + 1) + n * 2
        yield "prompt K/V B=4 S=4096 Hk=8 into a cache, the cache's (static) scales", ours_static, parent_static, n * 3
    if "config3" in which:
        B, S, H3 = 4, 4096, 32
        q, k, v = (torch.randn(B, S, H3, D, device=DEV, dtype=torch.bfloat16) for _ in range(3))
        yield ("config 3 q/k/v B=4 S=4096 H=32/32 D=128 (for the record: not a prefill speed-up)", lambda: quantize_fp8(q, k, v, num_heads_k=H3),
               lambda: [quant_dynamic(t, H3) for t in (q, k, v)], 3 * q.numel() * 5)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rows", default="decode,prompt,config3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_quant.py measures on the GPU only"
    lines = [f"# tools/bench_quant.py --steps {a.steps} --reps {a.reps}: us per step, median [min .. max] of {a.reps} windows of {a.steps} steps; {torch.cuda.get_device_name(0)}",
             "# ours = libfa_gfx950_quant.so; parent = PyTorch composition (tools/bench_decode.py quant()) + the e4m3 fa_kvcache_append; sides alternate window by window",
             f"# GB/s = bytes the algorithm must move / graph time (streaming kernels achieve about {HBM_TBS} TB/s on this part)"]
    for label, ours, parent, nbytes in rows(a.rows.split(",")):
        steps = a.steps if nbytes < (1 << 28) else max(2, a.steps // 5)
        with torch.no_grad():
            n_ours, n_parent = count_launches(ours), count_launches(parent)
            for f in (ours, parent):
                for _ in range(5):
                    f()
            torch.cuda.synchronize()
            g_ours, g_parent = make_graph(ours, steps), make_graph(parent, steps)
            t = {"ours eager": [], "parent eager": [], "ours graph": [], "parent graph": []}
            for _ in range(a.reps):   # alternate the sides
                t["ours eager"] += time_eager(ours, steps, 1)
                t["parent eager"] += time_eager(parent, steps, 1)
                t["ours graph"] += time_graph(g_ours, steps, 1)
                t["parent graph"] += time_graph(g_parent, steps, 1)
            del g_ours, g_parent
        lines.append(f"\n{label}")
        for side, n in (("ours", n_ours), ("parent", n_parent)):
            lines.append(f"  {side:6s} launches/step {n if n is not None else 'not counted':>3}   eager us {fmt(t[side + ' eager'])}   graph us {fmt(t[side + ' graph'])}")
        mo, mp = statistics.median(t["ours graph"]), statistics.median(t["parent graph"])
        lines.append(f"  ours moves {nbytes / 1e6:.2f} MB -> {nbytes / mo / 1e3:.1f} GB/s;  parent / ours: graph {mp / mo:.2f}x, eager {statistics.median(t['parent eager']) / statistics.median(t['ours eager']):.2f}x")
        print("\n".join(lines[-4:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
