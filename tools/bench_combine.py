"""Merge of partial attention results: libfa_gfx950_combine.so (flash_attn_combine / merge_attn_states) against the PyTorch composition a user writes without
it -- mask the infinite lse, max, exp, sum, divide, scale, add, cast: about eight element-wise launches with fp32 temporaries -- in this process, alternating
window by window, on the same inputs.

  prefill   pairwise bf16 merge of 16k and 128k tokens at H = 32 and H = 128, D = 128 (out (T, H, D), lse (H, T));
  decode    combine of fp32 partials at B*H = 128 / 512 / 2048 rows with 8 / 32 / 128 splits, D = 128 and 512, all partials live and the second half empty.

Per row: us per call, median [min .. max] of --reps windows of --steps calls (HIP events around the loop, after warm-up); bytes = what the algorithm has to
move, from the shapes: every lse, the o rows of the LIVE partials, the out and lse written; TB/s = bytes / median time, and its share of the 6.3 TB/s a
streaming kernel achieves on this part.  Kernel-only times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_combine.py --steps 3 --reps 2`.

usage: python tools/bench_combine.py [--steps 10] [--reps 9] [--rows prefill,decode] [--out profiles/combine_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention_amd"))
import torch  # noqa: E402

from flash_attn_amd import _cabi_combine, flash_attn_combine, merge_attn_states  # noqa: E402

DEV = "cuda"
HBM_TBS = 6.3
INF = float("inf")


def torch_merge(oa, la, ob, lb):
    """(T, H, D) / (H, T) pairwise merge as a user composes it; +-inf marks an empty side."""
    la, lb = la.transpose(0, 1), lb.transpose(0, 1)
    la, lb = torch.where(torch.isfinite(la), la, -INF), torch.where(torch.isfinite(lb), lb, -INF)
    m = torch.maximum(la, lb)
    m = torch.where(torch.isfinite(m), m, 0.0)
    ea, eb = torch.exp(la - m), torch.exp(lb - m)
    s = ea + eb
    out = (oa.float() * (ea / s).unsqueeze(-1) + ob.float() * (eb / s).unsqueeze(-1)).to(oa.dtype)
    return out, (m + torch.log(s)).transpose(0, 1).contiguous()


def torch_combine(op, lp):
    """(S, rows, H, D) / (S, rows, H) combine as a user composes it."""
    lp = torch.where(torch.isfinite(lp), lp, -INF)
    m = lp.amax(0)
    m = torch.where(torch.isfinite(m), m, 0.0)
    e = torch.exp(lp - m)
    s = e.sum(0)
    out = (op * (e / s).unsqueeze(-1)).sum(0)
    return out, m + torch.log(s)


def time_window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def fmt(ts):
    return f"{statistics.median(ts):9.1f} [{min(ts):8.1f} .. {max(ts):8.1f}]"


def rows(which):
    """(label, ours, composition, algorithmic bytes)"""
    torch.manual_seed(0)
    if "prefill" in which:
        D = 128
        for T, H in ((16384, 32), (131072, 32), (16384, 128), (131072, 128)):
            oa, ob = (torch.randn(T, H, D, device=DEV, dtype=torch.bfloat16) for _ in range(2))
            la, lb = (torch.randn(H, T, device=DEV) * 3 for _ in range(2))
            out, lse = torch.empty_like(oa), torch.empty_like(la)
            nbytes = 3 * oa.numel() * 2 + 3 * la.numel() * 4
            yield (f"prefill pair bf16 T={T} H={H} D={D}", lambda oa=oa, la=la, ob=ob, lb=lb, out=out, lse=lse: merge_attn_states(oa, la, ob, lb, out=out, lse=lse),
                   lambda oa=oa, la=la, ob=ob, lb=lb: torch_merge(oa, la, ob, lb), nbytes)
            del oa, ob, la, lb, out, lse
    if "decode" in which:
        for D in (128, 512):
            for R in (128, 512, 2048):
                for S in (8, 32, 128):
                    for half in (False, True):
                        op, lp = torch.randn(S, R, 1, D, device=DEV), torch.randn(S, R, 1, device=DEV) * 3
                        if half:
                            lp[S // 2:] = -INF
                        live = S // 2 if half else S
                        nbytes = live * R * D * 4 + S * R * 4 + R * D * 4 + R * 4
                        yield (f"decode fp32 rows={R} S={S} D={D}{' half empty' if half else ''}", lambda op=op, lp=lp: flash_attn_combine(op, lp),
                               lambda op=op, lp=lp: torch_combine(op, lp), nbytes)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rows", default="prefill,decode")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_combine.py measures on the GPU only"
    lines = [f"# tools/bench_combine.py --steps {a.steps} --reps {a.reps}: us per call, median [min .. max] of {a.reps} windows of {a.steps} calls; {torch.cuda.get_device_name(0)}",
             "# ours = libfa_gfx950_combine.so (one launch); torch = the PyTorch composition; the sides alternate window by window",
             f"# bytes = every lse + the o rows of the live partials + out + lse written; share = bytes / time / {HBM_TBS} TB/s",
             f"# {'shape':48s} {'kernel':26s} {'ours us':>30s} {'torch us':>30s} {'MB':>9s} {'TB/s':>6s} {'share':>6s} {'torch/ours':>10s}"]
    print("\n".join(lines), flush=True)
    with torch.no_grad():
        for label, ours, comp, nbytes in rows(a.rows.split(",")):
            for f in (ours, comp):
                for _ in range(3):
                    f()
            ours()
            kernel = _cabi_combine.last_kernel_name()
            torch.cuda.synchronize()
            t_ours, t_comp = [], []
            for _ in range(a.reps):
                t_ours.append(time_window(ours, a.steps))
                t_comp.append(time_window(comp, a.steps))
            mo, mc = statistics.median(t_ours), statistics.median(t_comp)
            tbs = nbytes / mo / 1e6
            lines.append(f"{label:50s} {kernel:26s} {fmt(t_ours)} {fmt(t_comp)} {nbytes / 1e6:9.2f} {tbs:6.2f} {tbs / HBM_TBS:6.1%} {mc / mo:10.2f}")
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
