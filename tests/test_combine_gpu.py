"""flash_attn_combine / merge_attn_states on the GPU (libfa_gfx950_combine.so): the reference's acceptance fixture under the reference's tolerance rule, the
empty-partial rules (nothing of an empty partial is read), the lse range, strided layouts bit for bit, the in-place running merge, both kernels, merges of real
kernel outputs against the oracle (with the per-chunk backward recipe), and a HIP-graph capture.  Tiny tensors: the whole module takes a few seconds.

The tolerance rule (reference hopper/test_flash_attn.py, test_flash_attn_combine): lse allclose(atol = rtol = 1e-5), equal infinities equal;
max|out - ref| <= 2 max|ref.to(dtype) - ref|, or allclose(1e-5) to ref.to(dtype)  (tests/_combine_ref.py within_reference_rule)."""
import os

import numpy as np
import pytest
import torch

from tests import _layouts as L
from tests._combine_ref import combine_ref64, load_cases, within_reference_rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
CASES = load_cases(os.path.join(ROOT, "tests", "golden", "combine_ref_cases.npz"))
INF = float("inf")
ROWS, SPLITS = "fa_combine_rows_kernel", "fa_combine_splits_kernel"


@pytest.fixture(scope="module")
def fa():
    import flash_attn_amd
    from flash_attn_amd import _cabi_combine, combine
    _cabi_combine.load()
    return flash_attn_amd, combine, _cabi_combine


@pytest.fixture(params=[1, 2], ids=["rows_kernel", "splits_kernel"])
def path(request, fa, monkeypatch):
    """Both kernels take every valid call: the tests that do not care about the shape-driven choice run on each."""
    monkeypatch.setattr(fa[1], "_PATH", request.param)
    return (ROWS, SPLITS)[request.param - 1]


def _rand(shape, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _assert_rule(out, lse, out_ref, lse_ref, dtype, what):
    ok, fig = within_reference_rule(out, lse, out_ref, lse_ref, dtype)
    print(f"{what}: out err {fig['out_err']:.3e} (rounding of the reference {fig['rounding']:.3e}) lse err {fig['lse_err']:.3e}")
    assert ok, (what, fig)


# ---- 1. the reference's fixture -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_cases(fa, name):
    """Inputs non-contiguous the way the reference's test builds them; 3 partial dtypes x 3 out dtypes.  fp32 partials: the stored results of the reference's
    oracle; 16-bit partials: the float64 formula on the rounded partials (tests/test_combine_cpu.py shows the two agree on the fixture)."""
    c = CASES[name]
    S, B, Ls, H, D = c["out_partial"].shape
    for pd in DTYPES:
        op, lp = torch.from_numpy(c["out_partial"]).to(pd), torch.from_numpy(c["lse_partial"])
        out_ref, lse_ref = (c["out"], c["lse"]) if pd == torch.float32 else combine_ref64(op, lp)
        ov = torch.full((2 * S, B, H, Ls, D), float("nan"), dtype=pd, device=DEV).transpose(2, 3)[:S]
        lv = torch.full((S, B, 2 * H, Ls), float("nan"), device=DEV).transpose(-1, -2)[:, :, :, :H]
        ov.copy_(op), lv.copy_(lp)
        for od in DTYPES:
            out, lse = fa[0].flash_attn_combine(ov, lv, out_dtype=od)
            assert out.dtype == od and out.shape == (B, Ls, H, D) and out.is_contiguous()
            assert lse.shape == (B, Ls, H) and lse.transpose(-1, -2).is_contiguous()
            _assert_rule(out, lse, out_ref, lse_ref, od, f"{name} {pd} -> {od} [{fa[2].last_kernel_name()}]")
    out2, none = fa[0].flash_attn_combine(ov, lv, return_lse=False)
    assert none is None and _same_bits(out2, fa[0].flash_attn_combine(ov, lv)[0])


# ---- 2. empty partials ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_empty_partials_are_not_read(fa, path, dtype):
    S, B, Ls, H, D = 5, 2, 7, 3, 64
    op, lp = _rand((S, B, Ls, H, D), 1, dtype), _rand((S, B, Ls, H), 2)
    g = torch.Generator().manual_seed(3)
    kind = torch.randint(0, 4, lp.shape, generator=g)                      # 0, 1: live; 2: -inf; 3: +inf
    kind[:, 0, :3] = torch.tensor([2, 3, 2, 3, 3])[:, None, None]          # rows without a live partial, both markers mixed
    kind[:, 1, 0] = torch.tensor([2, 2, 0, 3, 3])[:, None]                 # rows with exactly one live partial
    lp = torch.where(kind == 2, -INF, torch.where(kind == 3, INF, lp))
    empty = (kind >= 2)[..., None].expand_as(op)
    nan, zero = torch.where(empty, float("nan"), op.float()).to(dtype), torch.where(empty, 0.0, op.float()).to(dtype)
    out_n, lse_n = fa[0].flash_attn_combine(nan.to(DEV), lp.to(DEV))
    assert fa[2].last_kernel_name() == path
    out_z, lse_z = fa[0].flash_attn_combine(zero.to(DEV), lp.to(DEV))
    assert bool(torch.isfinite(out_n).all()) and _same_bits(out_n, out_z) and _same_bits(lse_n, lse_z)
    assert bool((out_n[0, :3] == 0).all()) and bool(torch.isneginf(lse_n[0, :3]).all())        # exactly 0 and exactly the asked infinity
    assert _same_bits(out_n[1, 0], op[2, 1, 0].to(DEV)) and torch.equal(lse_n[1, 0], lp[2, 1, 0].to(DEV))     # one live partial: reproduced exactly
    out_ref, lse_ref = combine_ref64(zero, lp)
    _assert_rule(out_n, lse_n, out_ref, lse_ref, dtype, f"empty partials {dtype} {path}")

    # the pairwise merge in the native layouts: +inf is this library's own marker
    a, b = _rand((B, Ls, H, D), 4, dtype), _rand((B, Ls, H, D), 5, dtype)
    la, lb = _rand((B, H, Ls), 6), _rand((B, H, Ls), 7)
    ka, kb = torch.randint(0, 3, la.shape, generator=g), torch.randint(0, 3, la.shape, generator=g)     # 0: live, 1: +inf, 2: -inf
    ka[0, 0, :2], kb[0, 0, :2] = torch.tensor([1, 2]), torch.tensor([1, 1])                            # both empty
    ka[0, 1, 0], kb[0, 1, 0] = 0, 1                                                                     # only a live
    la, lb = (torch.where(k == 1, INF, torch.where(k == 2, -INF, l)) for k, l in ((ka, la), (kb, lb)))
    ea, eb = ((k > 0).transpose(1, 2)[..., None].expand_as(a) for k in (ka, kb))
    args = lambda fill: (torch.where(ea, fill, a.float()).to(dtype).to(DEV), la.to(DEV), torch.where(eb, fill, b.float()).to(dtype).to(DEV), lb.to(DEV))
    out_n, lse_n = fa[0].merge_attn_states(*args(float("nan")))
    assert fa[2].last_kernel_name() == path
    out_z, lse_z = fa[0].merge_attn_states(*args(0.0))
    assert bool(torch.isfinite(out_n).all()) and _same_bits(out_n, out_z) and _same_bits(lse_n, lse_z)
    assert bool((out_n[0, :2, 0] == 0).all()) and bool(torch.isposinf(lse_n[0, 0, :2]).all())
    assert _same_bits(out_n[0, 0, 1], a[0, 0, 1].to(DEV)) and lse_n[0, 1, 0].item() == la[0, 1, 0].item()
    out_ref, lse_ref = combine_ref64(torch.stack([torch.where(ea, 0.0, a.float()), torch.where(eb, 0.0, b.float())]),
                                     torch.stack([la, lb]).transpose(-1, -2), empty=np.inf)
    _assert_rule(out_n, lse_n.transpose(1, 2), out_ref, lse_ref, dtype, f"empty partials, merge {dtype} {path}")


# ---- 3. range ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lse_range(fa, path, dtype):
    """lse = 30 randn, shifted by +-80 per row: exp() of an lse itself overflows fp32 at 88.7 -- only differences to the row's maximum may be exponentiated."""
    S, B, Ls, H, D = 6, 2, 33, 4, 64
    op, lp = _rand((S, B, Ls, H, D), 11, dtype), _rand((S, B, Ls, H), 12, scale=30.0)
    g = torch.Generator().manual_seed(13)
    lp = lp + (torch.randint(0, 2, (B, Ls, H), generator=g) * 160.0 - 80.0)
    lp[:, 0, :5] = -INF
    lp[3, 0, :5] = _rand((5, H), 14, scale=30.0) + 80.0                    # rows with one live partial
    out, lse = fa[0].flash_attn_combine(op.to(DEV), lp.to(DEV))
    assert fa[2].last_kernel_name() == path
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
    out_ref, lse_ref = combine_ref64(op, lp)
    _assert_rule(out, lse, out_ref, lse_ref, dtype, f"range {dtype} {path}")
    assert _same_bits(out[0, :5], op[3, 0, :5].to(DEV)) and torch.equal(lse[0, :5], lp[3, 0, :5].to(DEV))


# ---- 4. layouts -------------------------------------------------------------------------------------------------------------------------------------------------
def _batch_slice(data):
    """data as entries 1 .. B of a NaN-filled tensor of B + 2 entries."""
    big = torch.full((data.shape[0] + 2,) + tuple(data.shape[1:]), float("nan"), dtype=data.dtype, device=DEV)
    big[1:-1].copy_(data)
    return big, big[1:-1]


LAYOUT_SETS = {
    # out_a, lse_a, out_b, lse_b, out, lse   (lse tensors are (B, H, S): _layouts places them as 3-D tensors; "t" = the (B, S, H) transpose, "slice" = a batch slice)
    "A": ("bhsd", "t", "row_skip", "row_skip", "padded_head", "sbhd"),
    "B": ("padded_head", "padded_head", "slice", "slice", "row_skip", "bhsd"),
    "C": ("sbhd", "bhsd", "bhsd", "t", "bhsd", "padded_head"),
}


def _place_in(layout, data):
    if layout == "slice":
        big, view = _batch_slice(data.to(DEV))
        return (big, _bits(big).clone()), view
    if layout == "t":                       # lse (B, H, S) as the transpose of a contiguous (B, S, H) tensor
        buf = data.to(DEV).transpose(1, 2).contiguous()
        return (buf, _bits(buf).clone()), buf.transpose(1, 2)
    arena, view = L.place(layout, data=data, device=DEV)
    return arena, view


def _unchanged(handle):
    return handle.unchanged() if isinstance(handle, L.Arena) else torch.equal(_bits(handle[0]), handle[1])


@pytest.mark.parametrize("which", sorted(LAYOUT_SETS))
@pytest.mark.parametrize("dtypes", [(torch.bfloat16, torch.float32, torch.bfloat16), (torch.float16, torch.bfloat16, torch.float32)], ids=["bf16_f32_bf16", "f16_bf16_f32"])
def test_strided_layouts_give_the_same_bits(fa, path, which, dtypes):
    B, S, H, D = 3, 9, 3, 40
    da, db, do = dtypes
    a, b, la, lb = _rand((B, S, H, D), 21, da), _rand((B, S, H, D), 22, db), _rand((B, H, S), 23), _rand((B, H, S), 24)
    la[0, 0, :2], lb[0, 0, 1:3] = INF, INF
    want_out = torch.empty((B, S, H, D), dtype=do, device=DEV)
    _, want_lse = fa[0].merge_attn_states(a.to(DEV), la.to(DEV), b.to(DEV), lb.to(DEV), out=want_out)
    assert fa[2].last_kernel_name() == path
    lay = LAYOUT_SETS[which]
    handles, views = zip(*(_place_in(l, t) for l, t in zip(lay[:4], (a, la, b, lb))))
    out_arena, out_v = L.place(lay[4], shape=(B, S, H, D), dtype=do, kind="output", device=DEV)
    lse_arena, lse_v = L.place(lay[5], shape=(B, H, S), dtype=torch.float32, kind="output", device=DEV)
    got_out, got_lse = fa[0].merge_attn_states(*views, out=out_v, lse=lse_v)
    torch.cuda.synchronize()
    assert got_out is out_v and got_lse is lse_v
    assert _same_bits(out_v, want_out) and _same_bits(lse_v, want_lse)
    assert out_arena.outside_intact() and lse_arena.outside_intact()
    assert all(_unchanged(h) for h in handles)


def test_strided_stack_and_misaligned_view(fa, path):
    S, B, Ls, H, D = 3, 2, 5, 2, 72
    op, lp = _rand((S, B, Ls, H, D), 31, torch.float16), _rand((S, B, Ls, H), 32)
    want, want_lse = fa[0].flash_attn_combine(op.to(DEV), lp.to(DEV))
    ov = torch.full((2 * S, B, H, Ls, D + 8), float("nan"), dtype=torch.float16, device=DEV).transpose(2, 3)[1::2, ..., :D]
    lv = torch.full((S, B, 2 * H, Ls), float("nan"), device=DEV).transpose(-1, -2)[:, :, :, H:]
    ov.copy_(op), lv.copy_(lp)
    got, got_lse = fa[0].flash_attn_combine(ov, lv)
    assert fa[2].last_kernel_name() == path and _same_bits(got, want) and _same_bits(got_lse, want_lse)
    # the packed form is the same kernel on (1, total) rows
    gp, gl = fa[0].flash_attn_combine(ov.reshape(S, B * Ls, H, D), lv.reshape(S, B * Ls, H))
    assert _same_bits(gp.view(B, Ls, H, D), want) and _same_bits(gl.reshape(B, Ls, H), want_lse) and gl.transpose(0, 1).is_contiguous()
    flat = torch.zeros(S * B * Ls * H * D + 8, dtype=torch.float16, device=DEV)
    off = flat[4:-4].view(S, B, Ls, H, D)                                  # 8 bytes into a 16-byte aligned allocation
    with pytest.raises(RuntimeError, match=r"fa_combine: src\[0\]\.o must be 16-byte aligned"):
        fa[0].flash_attn_combine(off, lp.to(DEV))
    assert fa[2].last_kernel_name() == ""
    with pytest.raises(RuntimeError, match=r"fa_combine: src\[0\]\.o: batch stride 740 .* multiple of 16 bytes"):
        fa[0].flash_attn_combine(torch.zeros(S, B, Ls, H * D + 4, dtype=torch.float16, device=DEV)[..., :H * D].view(S, B, Ls, H, D), lp.to(DEV))
    assert fa[2].last_kernel_name() == ""


# ---- 5. in place ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_in_place_running_merge(fa, path, dtype):
    B, S, H, D = 2, 37, 3, 40                                              # d = 40: 5 lanes per row, 12 rows per wave, 4 idle lanes
    a, b, la, lb = _rand((B, S, H, D), 41, dtype).to(DEV), _rand((B, S, H, D), 42, torch.bfloat16).to(DEV), _rand((B, H, S), 43).to(DEV), _rand((B, H, S), 44).to(DEV)
    la[0, 0, :3], lb[0, 0, 2:5] = INF, INF
    want, want_lse = fa[0].merge_attn_states(a, la, b, lb)
    acc, acc_lse = a.clone(), la.clone()
    got, got_lse = fa[0].merge_attn_states(acc, acc_lse, b, lb, out=acc, lse=acc_lse)
    assert got is acc and got_lse is acc_lse and _same_bits(acc, want) and _same_bits(acc_lse, want_lse)


def test_folding_partials_into_an_fp32_accumulator(fa, path):
    """An empty accumulator (out = 0, lse = +inf) takes four bf16 partials one by one, in place; the four-way flash_attn_combine is the reference."""
    B, S, H, D = 2, 19, 2, 128
    op, lp = _rand((4, B, S, H, D), 51, torch.bfloat16).to(DEV), _rand((4, B, H, S), 52, scale=3.0).to(DEV)
    lp[1, 0, 0, :4] = INF
    acc, acc_lse = torch.zeros((B, S, H, D), device=DEV), torch.full((B, H, S), INF, device=DEV)
    for i in range(4):
        fa[0].merge_attn_states(acc, acc_lse, op[i], lp[i], out=acc, lse=acc_lse)
    ref, ref_lse = fa[0].flash_attn_combine(op, lp.transpose(-1, -2), out_dtype=torch.float32)
    _assert_rule(acc, acc_lse.transpose(1, 2), ref.double().cpu().numpy(), ref_lse.double().cpu().numpy(), torch.float32, f"fold of four {path}")


# ---- 6. both regimes, as the shapes pick them ---------------------------------------------------------------------------------------------------------------------
def test_the_shapes_pick_the_kernel(fa):
    T, H, D = 4099, 1, 64                                                   # 2 partials, 4099 rows: 513 waves of 8 rows, 129 workgroups
    a, b, la, lb = _rand((T, H, D), 61, torch.bfloat16), _rand((T, H, D), 62, torch.bfloat16), _rand((H, T), 63, scale=4.0), _rand((H, T), 64, scale=4.0)
    out, lse = fa[0].merge_attn_states(a.to(DEV), la.to(DEV), b.to(DEV), lb.to(DEV))
    assert fa[2].last_kernel_name() == ROWS
    out_ref, lse_ref = combine_ref64(torch.stack([a, b]), torch.stack([la, lb]).transpose(-1, -2), empty=np.inf)
    _assert_rule(out, lse.transpose(0, 1), out_ref, lse_ref, torch.bfloat16, "2 partials x 4099 rows")
    S, rows, D = 200, 6, 128                                                # 6 rows, 200 partials: one workgroup per row, 16 slots
    op, lp = _rand((S, 1, 1, rows, D), 65), _rand((S, 1, 1, rows), 66, scale=4.0)
    lp[40:120, :, :, 1] = -INF
    out, lse = fa[0].flash_attn_combine(op.to(DEV), lp.to(DEV))
    assert fa[2].last_kernel_name() == SPLITS
    out_ref, lse_ref = combine_ref64(op, lp)
    _assert_rule(out, lse, out_ref, lse_ref, torch.float32, "200 partials x 6 rows")
    # the thresholds of the choice (include/fa_gfx950_combine.h): more than 8 partials, or at least 4 on fewer rows than fill the chip
    for S, rows, want in ((8, 8192, ROWS), (9, 8192, SPLITS), (4, 64, SPLITS), (3, 64, ROWS), (4, 8192, ROWS)):
        op, lp = torch.zeros((S, rows, 1, 64), device=DEV), torch.zeros((S, rows, 1), device=DEV)
        out, lse = fa[0].flash_attn_combine(op, lp)
        assert fa[2].last_kernel_name() == want, (S, rows)
        assert bool((out == 0).all()) and torch.allclose(lse, torch.full_like(lse, float(np.log(S))), atol=1e-6)


# ---- 7. real kernel outputs -------------------------------------------------------------------------------------------------------------------------------------
def _err(x, ref):
    return float(np.abs(x.detach().double().cpu().numpy() - ref).max())


def _lse_err(lse, ref):
    lse = lse.detach().double().cpu().numpy()
    assert np.array_equal(np.isposinf(lse), np.isposinf(ref))
    fin = np.isfinite(ref)
    return float(np.abs(lse[fin] - ref[fin]).max())


def test_causal_attention_from_key_chunks_with_backward(fa):
    """Causal self-attention from two key chunks and the module docstring's backward recipe, against the oracle's monolithic result under smoke()'s bounds."""
    from flash_attn_amd import flash_attn_func
    from flash_attn_amd.flash_attn_interface import _flash_attn_backward
    from oracle import attention_oracle as orc
    torch.manual_seed(71)
    B, S, H, Hk, D, Cn = 2, 256, 4, 2, 128, 128
    scale = D ** -0.5
    q = torch.randn(B, S, H, D, device=DEV, dtype=torch.bfloat16)
    k, v = torch.randn(B, S, Hk, D, device=DEV, dtype=torch.bfloat16), torch.randn(B, S, Hk, D, device=DEV, dtype=torch.bfloat16)
    do = torch.randn_like(q)
    k0, v0, k1, v1 = k[:, :Cn], v[:, :Cn], k[:, Cn:], v[:, Cn:]
    with torch.no_grad():
        o1, l1, _ = flash_attn_func(q, k1, v1, causal=True, return_attn_probs=True)          # bottom-right aligned: rows < C see no key of chunk 1
        assert bool(torch.isposinf(l1[:, :, :Cn]).all()) and bool((o1[:, :Cn] == 0).all()) and bool(torch.isfinite(l1[:, :, Cn:]).all())
        o0a, l0a, _ = flash_attn_func(q[:, :Cn], k0, v0, causal=True, return_attn_probs=True)
        o0b, l0b, _ = flash_attn_func(q[:, Cn:], k0, v0, causal=False, return_attn_probs=True)
        om, lm = torch.empty_like(q), torch.empty(B, H, S, device=DEV)
        fa[0].merge_attn_states(o0a, l0a, o1[:, :Cn], l1[:, :, :Cn], out=om[:, :Cn], lse=lm[:, :, :Cn])      # row-slice views in and out
        fa[0].merge_attn_states(o0b, l0b, o1[:, Cn:], l1[:, :, Cn:], out=om[:, Cn:], lse=lm[:, :, Cn:])
        assert _same_bits(om[:, :Cn], o0a) and _same_bits(lm[:, :, :Cn], l0a)                                # merged with an empty partial: exact
        mono_o, mono_l, _ = flash_attn_func(q, k, v, causal=True, return_attn_probs=True)

        def bwd(dout, qq, kk, vv, oo, ll, causal):
            dq, dk, dv = torch.empty_like(qq), torch.empty_like(kk), torch.empty_like(vv)
            _flash_attn_backward(dout, qq, kk, vv, oo, ll.contiguous(), dq, dk, dv, 0.0, scale, causal, -1, -1, 0.0, None, False, None)
            return dq.float(), dk.float(), dv.float()

        dq1, dk1, dv1 = bwd(do, q, k1, v1, om, lm, True)
        dq0a, dk0a, dv0a = bwd(do[:, :Cn], q[:, :Cn], k0, v0, om[:, :Cn], lm[:, :, :Cn], True)
        dq0b, dk0b, dv0b = bwd(do[:, Cn:], q[:, Cn:], k0, v0, om[:, Cn:], lm[:, :, Cn:], False)
        dq = dq1 + torch.cat([dq0a, dq0b], dim=1)
        dk, dv = torch.cat([dk0a + dk0b, dk1], dim=1), torch.cat([dv0a + dv0b, dv1], dim=1)
        mdq, mdk, mdv = bwd(do, q, k, v, mono_o, mono_l, True)
    o_ref, l_ref = orc.attention_fwd(q, k, v, scale, True)
    g_ref = orc.attention_bwd(do, q, k, v, None, None, scale, True)[:3]
    fig = dict(out=_err(om, o_ref), lse=_lse_err(lm, l_ref), grads=[_err(g, r) for g, r in zip((dq, dk, dv), g_ref)])
    mono = dict(out=_err(mono_o, o_ref), lse=_lse_err(mono_l, l_ref), grads=[_err(g, r) for g, r in zip((mdq, mdk, mdv), g_ref)])
    print(f"combine-real causal chunks: merged {fig} monolithic {mono}")
    assert fig["out"] < 2e-2 and fig["lse"] < 2e-3 and max(fig["grads"]) < 6e-2, fig


def test_chunked_context_of_the_192_128_varlen_forward(fa):
    """Two context chunks of a packed batch through the (192, 128) varlen forward, one sequence empty in the second chunk, merged in (total, H, 128) / (H, total)."""
    from flash_attn_amd import flash_attn_varlen_func
    from oracle import attention_oracle as orc
    torch.manual_seed(72)
    H, Hk, D, DV = 4, 2, 192, 128
    scale = D ** -0.5
    lens_q, lens_k = [37, 5, 20], ([64, 30, 50], [40, 0, 17])
    cu = lambda lens: torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)
    q = torch.randn(sum(lens_q), H, D, device=DEV, dtype=torch.bfloat16)
    ks = [torch.randn(sum(l), Hk, D, device=DEV, dtype=torch.bfloat16) for l in lens_k]
    vs = [torch.randn(sum(l), Hk, DV, device=DEV, dtype=torch.bfloat16) for l in lens_k]
    with torch.no_grad():
        parts = [flash_attn_varlen_func(q, kc, vc, cu(lens_q), cu(l), max(lens_q), max(l), softmax_scale=scale, return_attn_probs=True)[:2]
                 for kc, vc, l in zip(ks, vs, lens_k)]
        (oa, la), (ob, lb) = parts
        s1 = slice(lens_q[0], lens_q[0] + lens_q[1])
        assert oa.shape == (sum(lens_q), H, DV) and la.shape == (H, sum(lens_q)) and bool(torch.isposinf(lb[:, s1]).all())
        om, lm = fa[0].merge_attn_states(oa, la, ob, lb)
        assert _same_bits(om[s1], oa[s1]) and _same_bits(lm[:, s1], la[:, s1])
        # the monolithic call: every sequence's two chunks concatenated
        seq = lambda ts, lens_pair, b: [t[sum(l[:b]):sum(l[:b + 1])] for t, l in zip(ts, lens_pair)]
        kcat = torch.cat([x for b in range(3) for x in seq(ks, lens_k, b)])
        vcat = torch.cat([x for b in range(3) for x in seq(vs, lens_k, b)])
        tot = [a + b for a, b in zip(*lens_k)]
        mono_o, mono_l = flash_attn_varlen_func(q, kcat, vcat, cu(lens_q), cu(tot), max(lens_q), max(tot), softmax_scale=scale, return_attn_probs=True)[:2]
    vpad = torch.nn.functional.pad(vcat, [0, D - DV])                      # the oracle takes one head dim: zero channels 128 .. 191 of V change nothing
    o_ref, l_ref = orc.varlen_fwd(q, kcat, vpad, cu(lens_q), cu(tot), scale)
    o_ref = o_ref[..., :DV]
    fig = dict(out=_err(om, o_ref), lse=_lse_err(lm, l_ref))
    mono = dict(out=_err(mono_o, o_ref), lse=_lse_err(mono_l, l_ref))
    print(f"combine-real 192/128 varlen chunks: merged {fig} monolithic {mono}")
    assert fig["out"] < 2e-2 and fig["lse"] < 2e-3, fig


def test_kv_cache_decode_step_from_two_halves(fa):
    """One decode step with the cache split in two by rows; one entry's cache_seqlens ends inside the first half: its second partial is empty."""
    from flash_attn_amd import flash_attn_with_kvcache
    from oracle import attention_oracle as orc
    torch.manual_seed(73)
    B, H, Hk, D, rows = 3, 4, 2, 128, 512
    scale = D ** -0.5
    q = torch.randn(B, 1, H, D, device=DEV, dtype=torch.bfloat16)
    kc, vc = torch.randn(B, rows, Hk, D, device=DEV, dtype=torch.bfloat16), torch.randn(B, rows, Hk, D, device=DEV, dtype=torch.bfloat16)
    lens = [400, 100, 512]
    half = rows // 2
    t32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=DEV)
    oa, la = flash_attn_with_kvcache(q, kc[:, :half], vc[:, :half], cache_seqlens=t32([min(n, half) for n in lens]), return_softmax_lse=True)
    ob, lb = flash_attn_with_kvcache(q, kc[:, half:], vc[:, half:], cache_seqlens=t32([max(n - half, 0) for n in lens]), return_softmax_lse=True)
    assert la.shape == (B, H, 1) and bool(torch.isinf(lb[1]).all()) and bool(torch.isfinite(lb[0]).all())
    om, lm = fa[0].merge_attn_states(oa, la, ob, lb)
    assert _same_bits(om[1], oa[1]) and _same_bits(lm[1], la[1])
    mono_o, mono_l = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=t32(lens), return_softmax_lse=True)
    refs = [orc.attention_fwd(q[b:b + 1], kc[b:b + 1, :n], vc[b:b + 1, :n], scale) for b, n in enumerate(lens)]
    o_ref, l_ref = np.concatenate([r[0] for r in refs]), np.concatenate([r[1] for r in refs])
    fig = dict(out=_err(om, o_ref), lse=_lse_err(lm, l_ref))
    mono = dict(out=_err(mono_o, o_ref), lse=_lse_err(mono_l, l_ref))
    print(f"combine-real kv-cache halves: merged {fig} monolithic {mono}")
    assert fig["out"] < 2e-2 and fig["lse"] < 2e-3, fig


# ---- 8. HIP graph, torch.compile ----------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay(fa):
    """One kernel, no parallel branches: captured once, replayed on new contents of the same buffers, equal to the eager call bit for bit."""
    B, S, H, D = 2, 50, 4, 128
    a, b = _rand((B, S, H, D), 81, torch.bfloat16).to(DEV), _rand((B, S, H, D), 82, torch.bfloat16).to(DEV)
    la, lb = _rand((B, H, S), 83).to(DEV), _rand((B, H, S), 84).to(DEV)
    out, lse = torch.empty_like(a), torch.empty_like(la)
    step = lambda: fa[0].merge_attn_states(a, la, b, lb, out=out, lse=lse)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                             # warm-up: loads the library and the code object outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for r in range(2):
        a.copy_(_rand((B, S, H, D), 85 + r, torch.bfloat16)), lb.copy_(_rand((B, H, S), 87 + r, scale=2.0))
        lb[0, 0, r] = INF
        out.zero_(), lse.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got, got_lse = out.clone(), lse.clone()
        want, want_lse = fa[0].merge_attn_states(a, la, b, lb)
        assert _same_bits(got, want) and _same_bits(got_lse, want_lse) and bool((got != 0).any())


def test_both_functions_compile_without_graph_breaks(fa):
    a, b = _rand((2, 9, 2, 64), 91, torch.bfloat16).to(DEV), _rand((2, 9, 2, 64), 92, torch.bfloat16).to(DEV)
    la, lb = _rand((2, 2, 9), 93).to(DEV), _rand((2, 2, 9), 94).to(DEV)
    merge = torch.compile(lambda *t: fa[0].merge_attn_states(*t), backend="eager", fullgraph=True)
    got, want = merge(a, la, b, lb), fa[0].merge_attn_states(a, la, b, lb)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    op, lp = torch.stack([a, b]), torch.stack([la, lb]).transpose(-1, -2)
    comb = torch.compile(lambda o, l: fa[0].flash_attn_combine(o, l, out_dtype=torch.float32), backend="eager", fullgraph=True)
    got, want = comb(op, lp), fa[0].flash_attn_combine(op, lp, out_dtype=torch.float32)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and got[1].stride() == want[1].stride()
