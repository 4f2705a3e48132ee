"""Learnable attention sinks on the GPU (flash_attn_amd/sink.py, libfa_gfx950_sink.so): the fixture of the reference's oracle through the autograd functions under the
reference's two rules, the post-pass and the dsink kernel alone against their float64 formulas, the bit-level promises (sink off, in place, strided layouts,
run-to-run), rows without a key with NaN poison where nothing may be read, decode, merge-then-sink, graph capture and torch.compile.  Tensors are tiny.
With FA_SINK_MARGINS=<path> the worst ratios of the fixture test are written there (profiles/sink_margins.txt is such a run)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import _layouts as lay
from tests import _sink_ref as sr
from tests._combine_ref import within_reference_rule

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
INF = math.inf
_MARGINS = {}


@pytest.fixture(scope="module")
def fa():
    import flash_attn_amd
    return flash_attn_amd


@pytest.fixture(scope="module")
def ops():
    import flash_attn_amd  # noqa: F401
    return torch.ops.flash_attn_amd


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    yield
    path = os.environ.get("FA_SINK_MARGINS")
    if path and _MARGINS:
        with open(path, "w") as f:
            f.write("# tests/test_sink_gpu.py test_fixture_under_the_reference_rules: worst error / allowance per quantity (in the rule iff <= 1; the torch stand-in with the\n"
                    "# kernels' roundings is held to 0.5 on the CPU), lse = worst |lse' - ref| (bound %.0e); over the sink dtypes fp32 and the inputs' own\n" % sr.LSE_TOL
                    + "# %-38s %-5s" % ("case", "dtype") + "".join("%9s" % q for q in sr.QUANTITIES + ("lse",)) + "\n")
            for (name, dn), m in sorted(_MARGINS.items()):
                f.write("%-40s %-5s" % (name, dn) + "".join("%9.3f" % m[q] for q in sr.QUANTITIES) + "%9.1e\n" % m["lse"])


def _dn(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp16"


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=DEV)


def _rand_result(shape_o, dtype, seed, lse_scale=3.0, dead_every=0):
    """A made-up attention result: out (.., S, H, D) in `dtype`, lse (.., H, S) fp32 (+inf on every dead_every-th row, whose out row is NaN)."""
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(shape_o, generator=g).to(dtype)
    lse = torch.randn(shape_o[:-3] + (shape_o[-2], shape_o[-3]), generator=g) * lse_scale
    if dead_every:
        dead = (torch.arange(lse.numel()).view(lse.shape) % dead_every) == 1
        lse[dead] = INF
        out[dead.transpose(-1, -2)] = math.nan
    sink = torch.randn(shape_o[-2], generator=g) * 2.0
    return out.to(DEV), lse.to(DEV), sink.to(DEV)


# ---- 1. the fixture ------------------------------------------------------------------------------------------------------------------------------------
def _run_case(fa, case, dtype, sink_dtype):
    m = sr.case_meta(case)
    q, k, v, do, sink = sr.case_inputs(case, dtype, DEV)
    sink = sink.to(sink_dtype)
    for t in (q, k, v, sink):
        t.requires_grad_(True)
    kw = dict(causal=m["causal"], window_size=m["window"], softcap=m["softcap"], return_attn_probs=True)
    if m["packed"]:
        out, lse, none = fa.flash_attn_varlen_sink_func(q, k, v, sink, _cu(m["qlens"]), _cu(m["klens"]), max(m["qlens"]), max(m["klens"]), **kw)
    else:
        out, lse, none = fa.flash_attn_sink_func(q, k, v, sink, **kw)
    assert none is None and not lse.requires_grad and out.dtype == dtype
    dq, dk, dv, dsink = torch.autograd.grad(out, (q, k, v, sink), do)
    assert dsink.dtype == sink_dtype and dsink.shape == sink.shape
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, dsink=dsink)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("name", sorted(sr.load_cases()))
def test_fixture_under_the_reference_rules(fa, name, dtype):
    """Every case of the reference's oracle, forward and backward, under check_tensor_vs_ref (out, dq, dk, dv) and check_dsink_vs_ref (dsink), with an fp32 sink
    and with a sink in the inputs' dtype; lse' within the project's bound for lse.

    Measured on the MI355X (profiles/sink_margins.txt is the last run): out, dq, dk, dv use 0.10 - 0.74 of their allowance, dsink 0.04 - 0.28, on every case and
    dtype.  dsink is the noise-limited quantity (one sum per head of the 16-bit rounding noise of out', against an allowance that is twice one realisation of the
    reference's own, smaller noise), which is why the fixture's generator keeps a case only if the stand-in stays within half of the allowance on sixteen
    realisations of that noise (tests/_sink_ref.py DSINK_VARIANTS, checked again in tests/test_sink_cpu.py).  The results are a function of the inputs alone:
    all six outputs of every case had the same bits over three calls with other work in between, and in two processes."""
    case = sr.load_cases()[name]
    worst = {}
    for sink_dtype in (torch.float32, dtype):
        res = sr.compare(case, _run_case(fa, case, dtype, sink_dtype), dtype, sink_dtype)
        print(name, _dn(dtype), "sink", sink_dtype, {k: float("%.3g" % x) for k, x in res.items()})
        for k_, x in res.items():
            worst[k_] = max(worst.get(k_, 0.0), x)
    _MARGINS[name, _dn(dtype)] = worst
    assert all(worst[q] <= 1.0 for q in sr.QUANTITIES), worst
    assert worst["lse"] < sr.LSE_TOL, worst


@pytest.mark.parametrize("name", ["gqa4_causal_113x203_d40", "pk_gqa2_causal_zero_d64"])
def test_results_are_a_function_of_the_inputs_alone(fa, name):
    """The same bits from call to call, with another shape's forward and backward and fresh allocations in between: what the fixture test measures is one number
    per tree, not a draw (dsink above all, which sums rounding noise and would show a schedule that depended on state)."""
    case = sr.load_cases()[name]
    first = _run_case(fa, case, torch.bfloat16, torch.float32)
    x = torch.randn(2, 512, 8, 128, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    fa.flash_attn_func(x, x, x, causal=True).float().sum().backward()
    junk = torch.full((1 << 20,), math.nan, device=DEV)
    del junk
    for _ in range(2):
        again = _run_case(fa, case, torch.bfloat16, torch.float32)
        assert all(torch.equal(first[k_], again[k_]) for k_ in first), [k_ for k_ in first if not torch.equal(first[k_], again[k_])]


def test_sink_that_needs_no_grad_skips_dsink_and_no_grad_mode_works(fa):
    case = sr.load_cases()["gqa4_causal_113x203_d40"]
    q, k, v, do, sink = sr.case_inputs(case, torch.bfloat16, DEV)
    q.requires_grad_(True)
    out = fa.flash_attn_sink_func(q, k, v, sink, causal=True)
    (dq,) = torch.autograd.grad(out, (q,), do)
    ref = _run_case(fa, case, torch.bfloat16, torch.float32)
    assert torch.equal(dq, ref["dq"]) and torch.equal(out, ref["out"])
    with torch.no_grad():
        out2 = fa.flash_attn_sink_func(q, k, v, sink, causal=True)
    assert torch.equal(out2, out) and not out2.requires_grad


# ---- 2. apply_attn_sink alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("shape", [(2, 37, 7, 8), (1, 100, 1, 40), (3, 65, 7, 64), (2, 130, 3, 128), (1, 67, 2, 512), (2, 1, 70, 64), (3, 3, 5, 128),
                                   (197, 7, 64), (1, 1, 128), (300, 1, 40)], ids=lambda s: "x".join(map(str, s)))
def test_apply_alone_against_the_float64_formula(fa, shape, dtype):
    """Both layouts; row counts that are no multiple of the 64-row tile; one head and seven; a decode step (s = 1: tiles of 64 heads) and s = 3 (tiles of 4 x 16);
    a sink dtype of each kind; every third row without a key, its out row NaN."""
    out, lse, sink = _rand_result(shape, dtype, seed=sum(shape), dead_every=3)
    for sink_dtype in (torch.float32, torch.bfloat16, torch.float16):
        s = sink.to(sink_dtype)
        o2, l2 = fa.apply_attn_sink(out, lse, s)
        ro, rl, _ = sr.apply_ref64(out.cpu(), lse.cpu(), s.cpu())
        ok, fig = within_reference_rule(o2, l2, ro, rl, dtype)
        assert ok, (sink_dtype, fig)
        dead = torch.isinf(lse)
        assert (o2[dead.transpose(-1, -2)] == 0).all() and torch.equal(l2[dead], s.float()[:, None].expand(lse.shape)[dead])
    assert o2.is_contiguous() and l2.is_contiguous() and l2.dtype == torch.float32


# ---- 3. sink off is bit-identical ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["default", "fused", "w64"])
def test_a_sink_of_minus_inf_is_the_identity_bit_for_bit(fa, knobs, route):
    from flash_attn_amd import backend as be
    if route == "fused":
        knobs.set("FA_BWD_MODE", 3)
    if route == "w64":
        knobs.set("FA_BWD_MODE", -1)
        knobs.set("FA_BWD_DQ_NW", 64)
    torch.manual_seed(3)
    B, Sq, Sk, H, Hk, D = (1, 300, 333, 2, 2, 128) if route != "default" else (2, 200, 77, 4, 2, 64)      # (default: Sq > Sk, rows without a key)
    q, k, v = (torch.randn(B, s, h, D, device=DEV, dtype=torch.bfloat16, requires_grad=True) for s, h in ((Sq, H), (Sk, Hk), (Sk, Hk)))
    do = torch.randn(B, Sq, H, D, device=DEV, dtype=torch.bfloat16)
    sink = torch.full((H,), -INF, device=DEV, requires_grad=True)
    out0, lse0, _ = fa.flash_attn_func(q, k, v, causal=True, return_attn_probs=True)
    g0 = torch.autograd.grad(out0, (q, k, v), do)
    out1, lse1, _ = fa.flash_attn_sink_func(q, k, v, sink, causal=True, return_attn_probs=True)
    *g1, dsink = torch.autograd.grad(out1, (q, k, v, sink), do)
    # the route, on this thread (the schedule record is per thread and autograd ran the backward on its own): the same call through the binder, same knobs
    be.bwd(do, q.detach(), k.detach(), v.detach(), out1.detach(), lse1, None, None, None, None, 0.0, D ** -0.5, True, -1, -1, 0.0, False, None, None)
    sched = be.last_schedule()
    if route == "fused":
        assert sched["bwd_spill"] == 3, sched
    if route == "w64":
        assert sched["bwd_spill"] == 0 and sched["bwd_dq_nw"] == 64, sched
    assert torch.equal(out0, out1) and torch.equal(lse0, lse1)
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
    assert torch.isfinite(dsink).all() and (dsink == 0).all()
    if route == "default":
        assert torch.isposinf(lse1).any()


# ---- 4. extremes -----------------------------------------------------------------------------------------------------------------------------------------
def test_extreme_sinks_and_lse_give_no_nan_and_no_inf(fa):
    out, lse, _ = _rand_result((2, 70, 4, 64), torch.bfloat16, seed=4)
    H = 4
    big = torch.full((H,), 80.0, device=DEV)
    o2, l2 = fa.apply_attn_sink(out, lse, big)
    assert float(o2.float().abs().max()) < 1e-25 and float((l2 - 80.0).abs().max()) <= 1e-5      # (|out| < 5, lse < 12: out' < 5 e^-68)
    o2, l2 = fa.apply_attn_sink(out, lse, -big)
    assert torch.equal(o2, out) and float((l2 - lse).abs().max()) <= 1e-5
    for sign in (1.0, -1.0):
        l60 = torch.full_like(lse, 60.0 * sign)
        s60 = torch.full((H,), -60.0 * sign, device=DEV)
        o2, l2 = fa.apply_attn_sink(out, l60, s60)
        assert torch.isfinite(o2.float()).all() and torch.isfinite(l2).all()
        assert float((l2 - 60.0).abs().max()) < 1e-5 * 60
        assert torch.equal(o2, out) if sign > 0 else float(o2.float().abs().max()) == 0.0      # exp(-120) is below fp32: the factor is exactly 1 or 0
        ro, rl, _ = sr.apply_ref64(out.cpu(), l60.cpu(), s60.cpu())
        assert within_reference_rule(o2, l2, ro, rl, torch.bfloat16)[0]
    # the same through the autograd functions: finite everywhere
    case = sr.load_cases()["gqa4_causal_113x203_d40"]
    q, k, v, do, _ = sr.case_inputs(case, torch.bfloat16, DEV)
    for t in (q, k, v):
        t.requires_grad_(True)
    for s in (80.0, -80.0):
        sink = torch.full((8,), s, device=DEV, requires_grad=True)
        out = fa.flash_attn_sink_func(q, k, v, sink, causal=True)
        grads = torch.autograd.grad(out, (q, k, v, sink), do)
        assert all(torch.isfinite(g.float()).all() for g in grads) and torch.isfinite(out.float()).all()


# ---- 5. rows without a key -----------------------------------------------------------------------------------------------------------------------------
def test_rows_without_a_key(fa, ops):
    torch.manual_seed(5)
    B, Sq, Sk, H, Hk, D = 2, 200, 77, 4, 2, 64
    dtype = torch.bfloat16
    q, k, v = (torch.randn(B, s, h, D, device=DEV, dtype=dtype, requires_grad=True) for s, h in ((Sq, H), (Sk, Hk), (Sk, Hk)))
    do = torch.randn(B, Sq, H, D, device=DEV, dtype=dtype)
    sink = torch.tensor([0.5, -1.0, 2.0, 0.0], device=DEV, requires_grad=True)
    out, lse, _ = fa.flash_attn_sink_func(q, k, v, sink, causal=True, return_attn_probs=True)
    dq, dk, dv, dsink = torch.autograd.grad(out, (q, k, v, sink), do)
    nokey = Sq - Sk
    assert (out[:, :nokey] == 0).all() and torch.equal(lse[:, :, :nokey], sink.detach()[None, :, None].expand(B, H, nokey))
    assert all(torch.isfinite(g.float()).all() for g in (dq, dk, dv, dsink)) and (dq[:, :nokey] == 0).all()
    # dsink == the float64 formula over the other rows, on the softmax_d = rowsum(dout * out') the backward works with
    delta = (do.double() * out.detach().double()).sum(-1).transpose(1, 2)                        # (B, H, Sq)
    lse_bwd = lse.clone()
    lse_bwd[:, :, :nokey] = INF
    ref, mag = sr.dsink_ref64(delta[:, :, nokey:].cpu(), lse[:, :, nokey:].cpu(), sink.detach().cpu())
    assert (np.abs(dsink.double().cpu().numpy() - ref) <= 1e-4 * mag + 1e-6).all(), (dsink, ref)   # (the kernels' softmax_d is an fp32 sum of D products)
    # NaN in the out rows of those rows, and in their softmax_d entries, reaches nothing
    with torch.no_grad():
        out0, lse0, _ = fa.flash_attn_func(q, k, v, causal=True, return_attn_probs=True)
        assert torch.isposinf(lse0[:, :, :nokey]).all()
        poisoned = out0.clone()
        poisoned[:, :nokey] = math.nan
        o2, l2 = fa.apply_attn_sink(poisoned, lse0, sink.detach())
        assert torch.equal(o2, out.detach()) and torch.equal(l2, lse)
        fa.apply_attn_sink(poisoned, lse0, sink.detach(), out_=poisoned, lse_=lse0)              # in place
        assert torch.equal(poisoned, out.detach()) and torch.equal(lse0, lse)
        d32 = delta.float().contiguous()
        a = ops._attn_sink_dsink(d32, lse_bwd, sink.detach())
        d32[:, :, :nokey] = math.nan
        b = ops._attn_sink_dsink(d32, lse_bwd, sink.detach())
        assert torch.equal(a, b) and torch.isfinite(b).all()
        assert (np.abs(b.double().cpu().numpy() - ref) <= 1e-5 * mag).all()


# ---- 6. the dsink kernel alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 63), (1, 1, 64), (3, 5, 65), (1, 64, 4096), (2, 5, 2048), (4, 1, 1000), (5, 1000), (64, 65), (1, 4096)],
                         ids=lambda s: "x".join(map(str, s)))
def test_dsink_kernel_alone(ops, shape):
    """(B, H, S) and (H, total) against the float64 formula: <= 1e-5 sum|terms| per head (fp32 sums in a tree: a few hundred eps of that at <= 4096 rows per head;
    one dropped row of typical size is ~1 / rows of it: far above).  Two calls give equal bits; strided softmax_d / lse_bwd give the bits of contiguous ones."""
    g = torch.Generator().manual_seed(sum(shape))
    H = shape[-2]
    sink = (torch.randn(H, generator=g) * 2).to(DEV)
    lse = (torch.randn(shape, generator=g) * 2)
    lse_bwd = torch.maximum(lse, sink.cpu()[:, None]) + torch.rand(shape, generator=g)        # lse' >= s
    dead = torch.rand(shape, generator=g) < 0.1
    lse_bwd[dead] = INF
    d = torch.randn(shape, generator=g)
    d[dead] = math.nan
    d, lse_bwd = d.to(DEV), lse_bwd.to(DEV)
    a = ops._attn_sink_dsink(d, lse_bwd, sink)
    b = ops._attn_sink_dsink(d, lse_bwd, sink)
    ref, mag = sr.dsink_ref64(d.cpu(), lse_bwd.cpu(), sink.cpu())
    assert a.dtype == torch.float32 and a.shape == (H,) and torch.equal(a, b) and torch.isfinite(a).all()
    err = np.abs(a.double().cpu().numpy() - ref)
    assert (err <= 1e-5 * mag).all(), (err, mag)
    if shape[-1] > 1:   # one dropped row would show
        terms = np.abs(np.where(np.isfinite(lse_bwd.cpu().numpy()), np.exp(sink.cpu().numpy()[:, None] - lse_bwd.cpu().numpy()) * np.nan_to_num(d.cpu().numpy()), 0.0))
        assert np.median(terms[terms > 0]) > 1e-5 * mag.max()
    # strided: the (.., S, H) transposes, and every second row of a wider buffer
    dt = d.transpose(-1, -2).contiguous().transpose(-1, -2)
    wide = torch.full(shape[:-1] + (2 * shape[-1] + 1,), math.nan, device=DEV)
    wide[..., 1::2] = lse_bwd
    c = ops._attn_sink_dsink(dt, wide[..., 1::2], sink)
    assert torch.equal(a, c)
    for sd in (torch.bfloat16, torch.float16):   # the sink in 16 bits: the same values after the cast
        e = ops._attn_sink_dsink(d, lse_bwd, sink.to(sd))
        assert torch.equal(e, ops._attn_sink_dsink(d, lse_bwd, sink.to(sd).float()))


# ---- 7. layouts ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("layout_in,layout_out", [("bhsd", "row_skip"), ("padded_head", "bhsd"), ("row_skip", "padded_head"), ("sbhd", "sbhd"), ("fused", "fused")])
@pytest.mark.parametrize("shape", [(2, 70, 3, 64), (150, 5, 40)], ids=["bshd", "packed"])
def test_apply_on_strided_layouts(fa, shape, layout_in, layout_out, dtype):
    out, lse, sink = _rand_result(shape, dtype, seed=7, dead_every=5)
    want_o, want_l = fa.apply_attn_sink(out, lse, sink)                                         # contiguous
    if layout_in == "fused":
        a_in, (src,) = lay.place_fused(datas=[out], spare_heads=2)
    else:
        a_in, src = lay.place(layout_in, data=out)
    if layout_out == "fused":
        a_out, (dst,) = lay.place_fused(shapes=[shape], dtype=dtype, kind="output", device=DEV, spare_heads=2)
    else:
        a_out, dst = lay.place(layout_out, shape=shape, dtype=dtype, kind="output", device=DEV)
    # lse: the (.., S, H) transpose as input, every second column of a wider sentinel buffer as output
    lse_in = lse.transpose(-1, -2).contiguous().transpose(-1, -2)
    wide = torch.full(lse.shape[:-1] + (2 * lse.shape[-1] + 1,), 12345.0, device=DEV)
    lse_out = wide[..., 1::2]
    o2, l2 = fa.apply_attn_sink(src, lse_in, sink, out_=dst, lse_=lse_out)
    assert o2 is dst and l2 is lse_out
    assert torch.equal(dst, want_o) and torch.equal(lse_out, want_l)                            # bit-identical to the contiguous call
    assert a_out.outside_intact() and a_in.unchanged() and (wide[..., 0::2] == 12345.0).all()   # sentinels intact, inputs untouched
    assert torch.equal(lse_in, lse)
    # in place on the strided view == out of place, bit for bit; nothing outside the view changes
    l_here = lse_in.clone().transpose(-1, -2).contiguous().transpose(-1, -2)
    fa.apply_attn_sink(src, l_here, sink, out_=src, lse_=l_here)
    assert torch.equal(src, want_o) and torch.equal(l_here, want_l) and a_in.outside_intact()


def test_a_misaligned_view_is_refused_and_nothing_is_written(fa):
    out, lse, sink = _rand_result((2, 20, 3, 64), torch.bfloat16, seed=8)
    buf = torch.zeros(2 * 20 * 3 * 64 + 8, device=DEV, dtype=torch.bfloat16)
    off = buf[4:4 + out.numel()].view(out.shape)                                                 # 8 bytes off
    dst = torch.full_like(out, 7.0)
    l_dst = torch.full_like(lse, 7.0)
    with pytest.raises(RuntimeError, match="out must be 16-byte aligned"):
        fa.apply_attn_sink(out, lse, sink, out_=off, lse_=l_dst)
    off.copy_(out)
    with pytest.raises(RuntimeError, match="out_in must be 16-byte aligned"):
        fa.apply_attn_sink(off, lse, sink, out_=dst, lse_=l_dst)
    odd = torch.zeros(2, 20, 3, 68, device=DEV, dtype=torch.bfloat16)[..., :64]                  # head stride 68 elements: 8 bytes off a multiple of 16
    with pytest.raises(RuntimeError, match="out: (row|head) stride .* multiple of 16 bytes"):
        fa.apply_attn_sink(out, lse, sink, out_=odd, lse_=l_dst)
    with pytest.raises(RuntimeError, match="lse overlaps lse_in"):
        fa.apply_attn_sink(out[:, :19], lse[:, :, :19], sink, out_=dst[:, :19], lse_=lse[:, :, 1:])                  # lse_ one row off lse
    torch.cuda.synchronize()
    assert (dst == 7.0).all() and (l_dst == 7.0).all() and (odd == 0).all() and (buf[:4] == 0).all() and (buf[-4:] == 0).all()


# ---- 8. varlen against fixed length -----------------------------------------------------------------------------------------------------------------------
def test_each_packed_sequence_matches_its_fixed_length_call(fa):
    """Within the rule, not bitwise: the packed and the per-sequence backward differ in rounding."""
    case = sr.load_cases()["pk_gqa2_causal_zero_d64"]
    m = sr.case_meta(case)
    dtype = torch.bfloat16
    got = _run_case(fa, case, dtype, torch.float32)
    q, k, v, do, sink = sr.case_inputs(case, dtype, DEV)
    dsink = torch.zeros_like(sink)
    for sq_, sk_ in sr.sequences(case):
        if sq_.stop == sq_.start:
            continue
        qs, ks, vs = (t[None].clone().requires_grad_(True) for t in (q[sq_], k[sk_], v[sk_]))
        s1 = sink.clone().requires_grad_(True)
        out, lse, _ = fa.flash_attn_sink_func(qs, ks, vs, s1, causal=m["causal"], window_size=m["window"], return_attn_probs=True)
        dq, dk, dv, ds = torch.autograd.grad(out, (qs, ks, vs, s1), do[None, sq_])
        dsink += ds
        key = "err_pt_bf16"
        for nm, a, b, sl in (("out", out[0], got["out"], sq_), ("dq", dq[0], got["dq"], sq_), ("dk", dk[0], got["dk"], sk_), ("dv", dv[0], got["dv"], sk_)):
            ref = torch.from_numpy(case[nm])[sl]
            allow = sr.tensor_allowance(ref, case[key][sr.QUANTITIES.index(nm)])
            assert float((a.detach().float() - b[sl].detach().float()).abs().max()) <= allow, nm
        assert float((lse[0] - got["lse"][:, sq_]).abs().max()) < sr.LSE_TOL
    allow = sr.dsink_allowance(torch.from_numpy(case["dsink"]), case["err_pt_bf16"][4], m["softcap"])
    assert ((dsink - got["dsink"]).abs().cpu() <= allow).all()


# ---- 9. decode -------------------------------------------------------------------------------------------------------------------------------------------
def _decode_oracle(q, kc, vc, lens, sink, causal=True):
    from oracle import attention_oracle as orc
    outs, lses = [], []
    for b in range(q.shape[0]):
        o, l = orc.attention_fwd(q[b:b + 1].cpu(), kc[b:b + 1, :lens[b]].cpu(), vc[b:b + 1, :lens[b]].cpu(), q.shape[-1] ** -0.5, causal)
        outs.append(o), lses.append(l)
    return sr.apply_ref64(np.concatenate(outs), np.concatenate(lses), sink.cpu())


@pytest.mark.parametrize("variant", ["contiguous", "paged", "split4", "gqa_packed", "append_batch_idx"])
def test_kvcache_sink_against_the_oracle(fa, knobs, variant):
    """flash_attn_with_kvcache_sink == the float64 oracle with the sink (the project's kv-cache bounds: out 2e-2, lse 2e-3), and == the float64 post-pass formula on
    the kernel's own (out, lse) under the combine module's rule."""
    from flash_attn_amd import backend as be
    torch.manual_seed(9)
    B, Sq, Sk, H, Hk, D = (2, 1, 515, 8, 2, 64)
    if variant == "gqa_packed":
        Sq, H, Hk = 3, 16, 2
    q = torch.randn(B, Sq, H, D, device=DEV, dtype=torch.bfloat16)
    kc, vc = (torch.randn(B, 768, Hk, D, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    lens = [515, 130]
    sink = torch.randn(H, device=DEV) * 2
    kw = dict(cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), causal=True)
    k_arg, v_arg, kl, vl = kc, vc, kc, vc
    if variant == "paged":
        page, per = 256, 3
        perm = torch.randperm(B * per, device=DEV)
        pool_k, pool_v = (torch.zeros(B * per + 1, page, Hk, D, device=DEV, dtype=torch.bfloat16) for _ in range(2))
        bt = (perm + 1).view(B, per).to(torch.int32)
        pool_k[bt.long().view(-1)] = kc.view(B * per, page, Hk, D)
        pool_v[bt.long().view(-1)] = vc.view(B * per, page, Hk, D)
        k_arg, v_arg, kw["block_table"] = pool_k, pool_v, bt
    if variant == "split4":
        kw["num_splits"] = 4
    if variant == "append_batch_idx":
        idx = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
        kw["cache_batch_idx"] = idx
        kw["k"], kw["v"] = (torch.randn(B, Sq, Hk, D, device=DEV, dtype=torch.bfloat16) for _ in range(2))
        kl, vl = kc[idx.long()].clone(), vc[idx.long()].clone()
        for b in range(B):
            kl[b, lens[b]:lens[b] + Sq], vl[b, lens[b]:lens[b] + Sq] = kw["k"][b], kw["v"][b]
        lens = [n + Sq for n in lens]
    out0, lse0 = fa.flash_attn_with_kvcache(q, k_arg, v_arg, return_softmax_lse=True, **kw)     # (an append writes the same rows every time)
    out, lse = fa.flash_attn_with_kvcache_sink(q, k_arg, v_arg, sink, return_softmax_lse=True, **kw)
    sched = be.last_schedule()
    if variant == "split4":
        assert sched["fwd_splits"] > 1, sched
    if variant == "gqa_packed":
        assert sched["fwd_pack"] == H // Hk, sched
    only = fa.flash_attn_with_kvcache_sink(q, k_arg, v_arg, sink, **kw)
    assert torch.equal(only, out)
    ro, rl, _ = sr.apply_ref64(out0.cpu(), lse0.cpu(), sink.cpu())
    ok, fig = within_reference_rule(out, lse, ro, rl, torch.bfloat16)
    assert ok, fig
    oo, ol, _ = _decode_oracle(q, kl, vl, lens, sink)
    assert float(np.abs(out.double().cpu().numpy() - oo).max()) < 2e-2 and float(np.abs(lse.double().cpu().numpy() - ol).max()) < 2e-3


def test_kvcache_sink_with_an_fp8_cache_and_descales(fa):
    """The fp8 cache's parity rule (tests/test_kvcache_fp8_gpu.py: 2 x the error of the e4m3-P emulation + 2 bf16 eps |ref|), on the sinked result."""
    from oracle import attention_oracle as orc
    from tests.test_kvcache_fp8_gpu import BF16_EPS, FP8, _dequant, _emulate
    g = torch.Generator().manual_seed(10)
    B, Sq, Sk, H, Hk, D = 2, 1, 300, 8, 2, 128
    q, kc, vc = ((torch.randn(s, generator=g)).to(FP8).to(DEV) for s in ((B, Sq, H, D), (B, Sk, Hk, D), (B, Sk, Hk, D)))
    qd, kd, vd = ((torch.rand(B, Hk, generator=g) * 1.9 + 0.05).to(DEV) for _ in range(3))
    sink = (torch.randn(H, generator=g) * 2).to(DEV)
    lens = torch.tensor([300, 77], dtype=torch.int32, device=DEV)
    out, lse = fa.flash_attn_with_kvcache_sink(q, kc, vc, sink, cache_seqlens=lens, causal=True, return_softmax_lse=True, q_descale=qd, k_descale=kd, v_descale=vd)
    assert out.dtype == torch.bfloat16
    for b, n in enumerate((300, 77)):
        qf, kf, vf = _dequant(q[b:b + 1].cpu(), qd[b:b + 1], Hk), _dequant(kc[b:b + 1, :n].cpu(), kd[b:b + 1], Hk), _dequant(vc[b:b + 1, :n].cpu(), vd[b:b + 1], Hk)
        ref_o, ref_l = orc.attention_fwd(qf, kf, vf, D ** -0.5, True, (-1, -1))
        emu = _emulate(qf, kf, vf, D ** -0.5, True, (-1, -1))
        ro, rl, _ = sr.apply_ref64(ref_o, ref_l, sink.cpu())
        eo, _, _ = sr.apply_ref64(emu, ref_l, sink.cpu())
        tol = 2 * np.abs(eo - ro).max() + 2 * BF16_EPS * np.abs(ro) + 1e-6
        assert (np.abs(out[b:b + 1].double().cpu().numpy() - ro) <= tol).all()
        assert float((np.abs(lse[b:b + 1].double().cpu().numpy() - rl) / np.maximum(1.0, np.abs(rl))).max()) < 5e-4


# ---- 10. merge, then sink ------------------------------------------------------------------------------------------------------------------------------
def test_merge_first_then_apply_the_sink_once(fa):
    case = sr.load_cases()["mha_full_64x300_d128"]
    dtype = torch.bfloat16
    q, k, v, _, sink = sr.case_inputs(case, dtype, DEV)
    sink = torch.full_like(sink, 6.0)                                                            # a sink that matters: lse ~ log(300) + 1/2, so it holds ~ 45 % of the mass
    with torch.no_grad():
        one, lse_one, _ = fa.flash_attn_sink_func(q, k, v, sink, return_attn_probs=True)
        parts = [fa.flash_attn_func(q, k[:, a:b], v[:, a:b], return_attn_probs=True)[:2] for a, b in ((0, 130), (130, 300))]
        mo, ml = fa.merge_attn_states(parts[0][0], parts[0][1], parts[1][0], parts[1][1])
        so, sl = fa.apply_attn_sink(mo, ml, sink)
        ref = torch.from_numpy(case["out"])
        allow = sr.tensor_allowance(ref, case["err_pt_bf16"][0])
        assert float((so.float() - one.float()).abs().max()) <= allow and float((sl - lse_one).abs().max()) < sr.LSE_TOL
        # the wrong order counts exp(s) twice: visibly different
        wrong = [fa.apply_attn_sink(o, l, sink) for o, l in parts]
        wo, wl = fa.merge_attn_states(wrong[0][0], wrong[0][1], wrong[1][0], wrong[1][1])
        assert float((wo.float() - one.float()).abs().max()) > 3 * allow and float((wl - lse_one).abs().min()) > 100 * sr.LSE_TOL


def test_out_of_place_call_leaves_the_inputs_version_counters_alone(fa):
    """Only what is written counts as mutated: an `out` that another autograd node saved for its backward stays usable after an out-of-place apply_attn_sink."""
    q, k, v = (torch.randn(1, 70, h, 64, device=DEV, dtype=torch.bfloat16, requires_grad=True) for h in (4, 2, 2))
    out, lse, _ = fa.flash_attn_func(q, k, v, causal=True, return_attn_probs=True)
    sink = torch.randn(4, device=DEV)
    o, l = out.detach(), lse.detach()
    vo, vl = o._version, l._version
    with torch.no_grad():
        fa.apply_attn_sink(o, l, sink)
        dst = torch.empty_like(o)
        fa.apply_attn_sink(o, l, sink, out_=dst)
    assert (o._version, l._version) == (vo, vl)
    out.float().sum().backward()                                                                # (out is saved for this backward)
    assert torch.isfinite(q.grad.float()).all()
    o2, l2 = o.clone(), l.clone()
    with torch.no_grad():
        fa.apply_attn_sink(o2, l2, sink, out_=o2, lse_=l2)
    assert o2._version > 0 and l2._version > 0 and torch.equal(o2, dst)                          # the in-place call does count


# ---- 11. graph capture ------------------------------------------------------------------------------------------------------------------------------------
def test_apply_and_dsink_capture_into_one_linear_graph(fa, ops):
    """No host synchronisation, no allocation outside the caching allocator: both ops capture on one stream (a linear graph) and replay on changed inputs."""
    out, lse, sink = _rand_result((2, 70, 4, 64), torch.bfloat16, seed=11, dead_every=7)
    d = torch.randn(2, 4, 70, device=DEV)
    o_dst, l_dst = torch.empty_like(out), torch.empty_like(lse)
    fa.apply_attn_sink(out, lse, sink, out_=o_dst, lse_=l_dst)                                   # warm-up: the library is loaded outside the capture
    ops._attn_sink_dsink(d, lse, sink)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.apply_attn_sink(out, lse, sink, out_=o_dst, lse_=l_dst)
        ds = ops._attn_sink_dsink(d, lse, sink)
    for seed in (12, 13):
        o_new, l_new, s_new = _rand_result((2, 70, 4, 64), torch.bfloat16, seed=seed, dead_every=7)
        out.copy_(o_new), lse.copy_(l_new), sink.copy_(s_new), d.normal_()
        graph.replay()
        torch.cuda.synchronize()
        eo, el = fa.apply_attn_sink(out, lse, sink)
        assert torch.equal(o_dst, eo) and torch.equal(l_dst, el) and torch.equal(ds, ops._attn_sink_dsink(d, lse, sink))


# ---- 12. torch.compile -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["aot_eager", "inductor"])
def test_compile_fullgraph_forward_and_backward_equal_eager(fa, backend):
    """aot_eager: dynamo + functionalisation + AOT autograd through the ops; inductor: what users run (its handling of the mutating op and its fallbacks)."""
    torch.manual_seed(12)
    q, k, v = (torch.randn(2, 128, h, 64, device=DEV, dtype=torch.bfloat16, requires_grad=True) for h in (4, 2, 2))
    sink = torch.randn(4, device=DEV, requires_grad=True)

    def f(q, k, v, sink):
        return fa.flash_attn_sink_func(q, k, v, sink, causal=True, window_size=(31, 0))

    out = f(q, k, v, sink)
    grads = torch.autograd.grad(out.float().sum(), (q, k, v, sink))
    fc = torch.compile(f, backend=backend, fullgraph=True)
    oc = fc(q, k, v, sink)
    gc = torch.autograd.grad(oc.float().sum(), (q, k, v, sink))
    assert torch.equal(out, oc) and all(torch.equal(a, b) for a, b in zip(grads, gc))
