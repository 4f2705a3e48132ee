"""Head dims (192, 128) -- q / k 192, v / o 128 -- against the route a user had before: V zero-padded to 192 through the head-dim-192
kernels (profiles/fwd_dv.txt).

    python tools/headdim_v_ab.py [--windows 7] [--steps 10] [--out profiles/fwd_dv.txt] [--b 2 --s 4096 --h 32 --hk 32]

One process, one GPU.  Routes, forward and backward each:
  dv         the new path: v (B, S, Hk, 128) as given (forward kernel fa_fwd_dv_kernel; backward: the 256-pitch kernels with value width 128);
  pad        V already padded to 192 (and dO padded, O 192 wide): the head-dim-192 kernels alone, no copies timed -- the baseline of the bars;
  pad+copy   what the caller really ran: pad V (and dO) to 192, run, slice out / dV back to 128 (contiguous).
After an untimed clock ramp and a warm-up of every route, the routes ALTERNATE: each window times `steps` launches of one route between two
device events, W windows per route.  Reported: the median window and the spread (max - min) / median of the windows.  FLOPs: the project's
convention, 2 * visible pairs * (D + Dv) per (batch, head) for the forward (the work the (192, 128) problem needs -- the padded route is
charged the same, it solves the same problem) and 2.5 x that for the backward.
Bars: the forward's median on dv must be at least as fast as on pad (it does 5/6 of the matrix work on a kernel that holds two workgroups per CU);
the backward on dv must not be slower than on pad by more than pad's window spread (it saves 1/6 of two of its contractions and nothing else)."""
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

D, DV = 192, 128


def visible_pairs(sq, sk, causal):
    if not causal:
        return sq * sk
    shift = sk - sq
    return sum(max(0, min(sk, i + shift + 1)) for i in range(sq))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--b", type=int, default=2)
    ap.add_argument("--s", type=int, default=4096)
    ap.add_argument("--h", type=int, default=32)
    ap.add_argument("--hk", type=int, default=32)
    ap.add_argument("--no-causal", action="store_true")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)
    assert a.windows >= 5, "at least 5 windows per route"
    if not torch.cuda.is_available():
        raise SystemExit("headdim_v_ab.py measures on the GPU: no device found")
    from flash_attn_amd import backend as be
    dev = torch.device("cuda", 0)
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    causal = not a.no_causal
    B, S, H, Hk = a.b, a.s, a.h, a.hk
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(B, S, H, D, device=dev, dtype=dt, generator=g)
    k = torch.randn(B, S, Hk, D, device=dev, dtype=dt, generator=g)
    v = torch.randn(B, S, Hk, DV, device=dev, dtype=dt, generator=g)
    do = torch.randn(B, S, H, DV, device=dev, dtype=dt, generator=g)
    sc = D ** -0.5
    pad = lambda t: torch.nn.functional.pad(t, (0, D - DV))
    vp, dop = pad(v), pad(do)

    fwd = lambda q_, k_, v_: be.fwd(q_, k_, v_, None, None, 0.0, sc, causal, -1, -1, 0.0, False, None)[:2]
    bwd = lambda do_, v_, o_, l_: be.bwd(do_, q, k, v_, o_, l_, None, None, None, None, 0.0, sc, causal, -1, -1, 0.0, False, None, None)[:3]
    names = {}
    out, lse = fwd(q, k, v)
    names["fwd dv"] = be.last_schedule()["name"]
    outp, lsep = fwd(q, k, vp)
    names["fwd pad"] = be.last_schedule()["name"]
    # same problem, same answer (the padded route's extra columns are zeros)
    err_o = float((out.float() - outp[..., :DV].float()).abs().max())
    g_dv = bwd(do, v, out, lse)
    sched_dv = be.last_schedule()
    g_pad = bwd(dop, vp, outp, lsep)
    sched_pad = be.last_schedule()
    err_g = [float((x.float() - y[..., :x.shape[-1]].float()).abs().max()) for x, y in zip(g_dv, g_pad)]

    routes = {
        "fwd dv": lambda: fwd(q, k, v),
        "fwd pad": lambda: fwd(q, k, vp),
        "fwd pad+copy": lambda: fwd(q, k, pad(v))[0][..., :DV].contiguous(),
        "bwd dv": lambda: bwd(do, v, out, lse),
        "bwd pad": lambda: bwd(dop, vp, outp, lsep),
        "bwd pad+copy": lambda: bwd(pad(do), pad(v), pad(out), lse)[2][..., :DV].contiguous(),
    }
    sync = torch.cuda.synchronize
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:   # clock ramp
        routes["fwd pad"]()
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
    fl_f = 2.0 * B * H * visible_pairs(S, S, causal) * (D + DV)
    lines = [f"# tools/headdim_v_ab.py: B={B} S={S} H={H} Hk={Hk} D={D} Dv={DV} {a.dtype} {'causal' if causal else 'no mask'}; "
             f"{a.windows} windows x {a.steps} launches per route, routes alternating; device {torch.cuda.get_device_name(0)}",
             f"# FLOPs: forward 2 * pairs * (D + Dv) = {fl_f:.4g}, backward 2.5 x; max |out dv - out pad| = {err_o:.3g}, "
             f"max |dq, dk, dv: dv - pad| = {err_g}",
             f"# kernels: fwd dv {names['fwd dv']} | fwd pad {names['fwd pad']} | bwd dv dq_nw={sched_dv['bwd_dq_nw']} dkdv_nw={sched_dv['bwd_dkdv_nw']} spill={sched_dv['bwd_spill']}"
             f" | bwd pad dq_nw={sched_pad['bwd_dq_nw']} dkdv_nw={sched_pad['bwd_dkdv_nw']} spill={sched_pad['bwd_spill']}"]
    res = {}
    for n, xs in ms.items():
        med = statistics.median(xs)
        spread = (max(xs) - min(xs)) / med
        fl = fl_f * (2.5 if n.startswith("bwd") else 1.0)
        res[n] = {"median_ms": round(med, 4), "spread": round(spread, 4), "tflops": round(fl / med / 1e9, 1),
                  "windows_ms": [round(x, 4) for x in xs]}
        lines.append(f"{n:13s} median {med:8.4f} ms  spread {100 * spread:5.1f} %  {fl / med / 1e9:7.1f} TFLOP/s   windows {res[n]['windows_ms']}")
    fwd_ok = res["fwd dv"]["median_ms"] <= res["fwd pad"]["median_ms"]
    bwd_ok = res["bwd dv"]["median_ms"] <= res["bwd pad"]["median_ms"] * (1.0 + res["bwd pad"]["spread"])
    lines.append(f"forward bar (dv >= pad without copies): {'MET' if fwd_ok else 'MISSED'}: dv / pad time = "
                 f"{res['fwd dv']['median_ms'] / res['fwd pad']['median_ms']:.3f}")
    lines.append(f"backward bar (dv not slower than pad by more than pad's spread {100 * res['bwd pad']['spread']:.1f} %): "
                 f"{'MET' if bwd_ok else 'MISSED'}: dv / pad time = {res['bwd dv']['median_ms'] / res['bwd pad']['median_ms']:.3f}")
    report = "\n".join(lines)
    print(report)
    print(json.dumps({"routes": res, "fwd_bar": fwd_ok, "bwd_bar": bwd_ok}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report + "\n")
    return res


if __name__ == "__main__":
    main()
