"""Attention sinks as a post-pass: libfa_gfx950_sink.so against what a user writes without it, in this process, the sides alternating window by window on the
same inputs.

  apply     fa_sink_apply in place on (out, lse) against (i) the PyTorch composition -- out * sigmoid(lse - s).transpose(1, 2)[..., None], cast back, copied
            into out, plus the lse update: at least three passes over out and fp32 temporaries -- and (ii) out.copy_(out2), the same bytes read and written by
            a plain copy, timed in the same run: the kernel moves the copy's traffic plus 8 bytes (4 for a 16-bit sink ... 12 with lse_bwd) per row of D elements.
            Shapes: B=4 S=4096 H=32 D=128, B=8 S=2048 H=16 D=64, a packed 64k-token H=16 D=128, and the decode steps B=64 / 256, Sq=1, H=64, D=64.
  attn      flash_attn_sink_func against flash_attn_func, causal bf16, forward and forward + backward, at the first two shapes; the difference beside the byte
            model: forward one read + one write of out and 12 bytes per row, backward two (B, H, S) fp32 reads.
  dsink     fa_sink_dsink alone at those shapes.

Per row: us per call, median [min .. max] of --reps windows of --steps calls (HIP events around the loop, after warm-up); bytes from the shapes; TB/s = bytes /
median time.  The working sets of the large shapes (134 MB, 67 MB) fit the 256 MiB Infinity Cache, for the copy as for the kernel: the ratio to the copy is the
figure to read, not the TB/s alone.

usage: python tools/bench_sink.py [--steps 20] [--reps 9] [--rows apply,graph,attn,dsink] [--out profiles/sink.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention_amd"))
import torch  # noqa: E402

from flash_attn_amd import apply_attn_sink, flash_attn_func, flash_attn_sink_func  # noqa: E402

DEV = "cuda"
HBM_TBS = 6.3
APPLY_SHAPES = [("B=4 S=4096 H=32 D=128", (4, 4096, 32, 128)), ("B=8 S=2048 H=16 D=64", (8, 2048, 16, 64)), ("packed T=65536 H=16 D=128", (65536, 16, 128)),
                ("decode B=64 Sq=1 H=64 D=64", (64, 1, 64, 64)), ("decode B=256 Sq=1 H=64 D=64", (256, 1, 64, 64))]
ATTN_SHAPES = APPLY_SHAPES[:2]


def torch_sink(out, lse, s, lse2):
    """The composition, out in place like the kernel: (B, S, H, D) / (B, H, S) or (T, H, D) / (H, T)."""
    f = torch.sigmoid(lse - s[:, None]).transpose(-1, -2)[..., None]
    out.copy_((out * f).to(out.dtype))
    lse2.copy_(torch.logaddexp(lse, s[:, None].expand_as(lse)))


def time_window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def fmt(ts):
    return f"{statistics.median(ts):8.1f} [{min(ts):7.1f} ..{max(ts):8.1f}]"


def measure(fns, steps, reps):
    """The sides of one row, alternating window by window -> list of lists of us."""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            ts[i].append(time_window(f, steps))
    return ts


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rows", default="apply,graph,attn,dsink")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_sink.py measures on the GPU only"
    which = a.rows.split(",")
    lines = [f"# tools/bench_sink.py --steps {a.steps} --reps {a.reps}: us per call, median [min .. max] of {a.reps} windows of {a.steps} calls; {torch.cuda.get_device_name(0)}",
             "# the sides of a row alternate window by window in one process; bytes from the shapes; TB/s = bytes / median time"]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    torch.manual_seed(0)
    ops = torch.ops.flash_attn_amd
    with torch.no_grad():
        if "apply" in which:
            emit("#\n# (a) fa_sink_apply in place | the PyTorch composition in place | out.copy_(out2): the same bytes as a plain copy")
            emit(f"# {'shape':30s} {'kernel us':>28s} {'composition us':>28s} {'copy us':>28s} {'MB':>8s} {'TB/s':>6s} {'of 6.3':>6s} {'comp/kernel':>11s} {'kernel/copy':>11s}")
            for label, shape in APPLY_SHAPES:
                out = torch.randn(shape, device=DEV, dtype=torch.bfloat16)
                out2 = torch.randn_like(out)
                lse = torch.randn(shape[:-3] + (shape[-2], shape[-3]), device=DEV) * 3
                s = torch.randn(shape[-2], device=DEV) * 2
                nbytes = 2 * out.numel() * 2 + 2 * lse.numel() * 4
                lse2 = torch.empty_like(lse)   # (lse' goes to a buffer of its own so that every call sees the same factors; out shrinks call by call, which no side's time depends on)
                tk, tc, tp = measure([lambda: apply_attn_sink(out, lse, s, out_=out, lse_=lse2), lambda: torch_sink(out, lse, s, lse2), lambda: out.copy_(out2)], a.steps, a.reps)
                mk, mc, mp = (statistics.median(t) for t in (tk, tc, tp))
                emit(f"{label:32s} {fmt(tk)} {fmt(tc)} {fmt(tp)} {nbytes / 1e6:8.2f} {nbytes / mk / 1e6:6.2f} {nbytes / mk / 1e6 / HBM_TBS:6.1%} {mc / mk:11.2f} {mk / mp:11.2f}")
                del out, out2, lse
                torch.cuda.empty_cache()
        if "graph" in which:
            emit(f"#\n# (d) the same two sides of (a) as KERNEL time: {a.steps} calls captured into one graph per side, us per call of a replay (no host work between the launches)")
            emit(f"# {'shape':30s} {'kernel us':>28s} {'copy us':>28s} {'MB':>8s} {'TB/s':>6s} {'kernel/copy':>11s}")
            for label, shape in APPLY_SHAPES:
                out = torch.randn(shape, device=DEV, dtype=torch.bfloat16)
                out2 = torch.randn_like(out)
                lse = torch.randn(shape[:-3] + (shape[-2], shape[-3]), device=DEV) * 3
                s = torch.randn(shape[-2], device=DEV) * 2
                lse2 = torch.empty_like(lse)
                nbytes = 2 * out.numel() * 2 + 2 * lse.numel() * 4
                apply_attn_sink(out, lse, s, out_=out, lse_=lse2)
                torch.cuda.synchronize()
                graphs = []
                for side in (lambda: apply_attn_sink(out, lse, s, out_=out, lse_=lse2), lambda: out.copy_(out2)):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for _ in range(a.steps):
                            side()
                    graphs.append(g)
                tk, tp = ([t / a.steps for t in ts] for ts in measure([graphs[0].replay, graphs[1].replay], 1, a.reps))
                mk, mp = statistics.median(tk), statistics.median(tp)
                emit(f"{label:32s} {fmt(tk)} {fmt(tp)} {nbytes / 1e6:8.2f} {nbytes / mk / 1e6:6.2f} {mk / mp:11.2f}")
                del graphs, out, out2, lse
                torch.cuda.empty_cache()
        if "dsink" in which:
            emit("#\n# (c) fa_sink_dsink (two launches, bit-reproducible) | the PyTorch composition -(exp(s - lse') * softmax_d).sum(rows)")
            emit(f"# {'shape':30s} {'kernel us':>28s} {'composition us':>28s} {'MB':>8s} {'TB/s':>6s} {'comp/kernel':>11s}")
            for label, shape in ATTN_SHAPES:
                B, S, H, _ = shape
                d, l, s = torch.randn(B, H, S, device=DEV), torch.randn(B, H, S, device=DEV) * 3 + 6, torch.randn(H, device=DEV) * 2
                nbytes = 2 * d.numel() * 4
                tk, tc = measure([lambda: ops._attn_sink_dsink(d, l, s), lambda: -(torch.exp(s[None, :, None] - l) * d).sum((0, 2))], a.steps, a.reps)
                mk, mc = statistics.median(tk), statistics.median(tc)
                emit(f"{label:32s} {fmt(tk)} {fmt(tc)} {nbytes / 1e6:8.2f} {nbytes / mk / 1e6:6.2f} {mc / mk:11.2f}")
    if "attn" in which:
        emit("#\n# (b) flash_attn_sink_func | flash_attn_func, causal bf16 (Hk = H); diff = what the sink costs, beside the byte model at 6.3 TB/s:")
        emit("#     extra bytes fwd = one read + one write of out + 8 B per row (lse read, lse' written; + 4 B lse_bwd when training), bwd = two (B, H, S) fp32 reads")
        emit(f"# {'shape':30s} {'pass':8s} {'with sink us':>28s} {'without us':>28s} {'diff us':>8s} {'extra MB':>9s} {'extra at 6.3 TB/s us':>20s}")
        for label, shape in ATTN_SHAPES:
            B, S, H, D = shape
            q, k, v = (torch.randn(B, S, H, D, device=DEV, dtype=torch.bfloat16, requires_grad=True) for _ in range(3))
            do = torch.randn(B, S, H, D, device=DEV, dtype=torch.bfloat16)
            s = (torch.randn(H, device=DEV) * 2).requires_grad_(True)

            def fwd_sink():
                with torch.no_grad():
                    flash_attn_sink_func(q, k, v, s, causal=True)

            def fwd_plain():
                with torch.no_grad():
                    flash_attn_func(q, k, v, causal=True)

            def both_sink():
                torch.autograd.grad(flash_attn_sink_func(q, k, v, s, causal=True), (q, k, v, s), do)

            def both_plain():
                torch.autograd.grad(flash_attn_func(q, k, v, causal=True), (q, k, v), do)

            rows = B * S * H
            for name, f1, f0, extra in (("fwd", fwd_sink, fwd_plain, 2 * rows * D * 2 + 8 * rows), ("fwd+bwd", both_sink, both_plain, 2 * rows * D * 2 + 12 * rows + 8 * rows)):
                t1, t0 = measure([f1, f0], a.steps, a.reps)
                m1, m0 = statistics.median(t1), statistics.median(t0)
                emit(f"{label:32s} {name:8s} {fmt(t1)} {fmt(t0)} {m1 - m0:8.1f} {extra / 1e6:9.2f} {extra / HBM_TBS / 1e6:20.1f}")
            del q, k, v, do
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
