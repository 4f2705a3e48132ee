"""GPU tests of a v / o head dim that differs from q / k: D = 192, Dv = 128 (DeepSeek-V2/V3 multi-head latent attention), forward
(csrc/fa_fwd_dv.hip, forward kernel id 6) and backward (the 256-pitch kernels of csrc/fa_bwd.hip with a value width of 128).

Reference being matched: the reference's newer interface takes "Q/K headdim in (128, 192] and V headdim in (96, 128]" as given
(hopper/flash_api.cpp:782-786 forward, :1345-1531 backward).  Tolerances: the rule of tests/test_headdim_trimmed_gpu.py::_check -- out within
2x the error of a same-dtype PyTorch evaluation against fp32 (+ 1e-4), gradients within 3x (+ 2e-4), LSE within 2e-3, +inf exactly where
no key is visible.  The NaN-guard tests prove that V / O / dO / dV are used in place: memory right behind their 128 columns is NaN (inputs)
or a sentinel (outputs)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests._util import attention_torch, max_abs

pytestmark = pytest.mark.gpu

D, DV = 192, 128
SCALE = D ** -0.5


@pytest.fixture(scope="module")
def be():
    from flash_attn_amd import backend
    return backend


def _ref(q, k, v, do, causal, window, upcast):
    qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o, l = attention_torch(qq, kk, vv, causal, window, upcast=upcast, reorder=not upcast)
    return (o, l) + torch.autograd.grad(o, (qq, kk, vv), do.to(o.dtype))


def _check(out, lse, grads, q, k, v, do, causal, window, what=""):
    """tests/test_headdim_trimmed_gpu.py::_check, printing each figure before it asserts."""
    o32, l32, q32, k32, v32 = _ref(q.float(), k.float(), v.float(), do.float(), causal, window, True)
    opt, _, qpt, kpt, vpt = _ref(q, k, v, do, causal, window, False)
    e, b = max_abs(out.float(), o32), max_abs(opt.float(), o32)
    print(f"{what} out err {e:.3e} (pytorch {b:.3e})")
    assert e <= 2 * b + 1e-4
    fin = torch.isfinite(l32)
    assert max_abs(lse[fin], l32[fin]) < 2e-3 and torch.equal(torch.isposinf(lse), ~fin)
    if grads is None:
        return
    for nm, got, r, p_ in zip(("dq", "dk", "dv"), grads, (q32, k32, v32), (qpt, kpt, vpt)):
        e, b = max_abs(got.float(), r), max_abs(p_.float(), r)
        print(f"{what} {nm} err {e:.3e} (pytorch {b:.3e})")
        assert got.shape == r.shape and e <= 3 * b + 2e-4


def _fwd(mod, q, k, v, causal=False, window=(-1, -1), out_=None, scale=SCALE):
    return mod.fwd(q, k, v, out_, None, 0.0, scale, causal, window[0], window[1], 0.0, False, None)[:2]


def _bwd(mod, do, q, k, v, out, lse, causal=False, window=(-1, -1), bufs=(None, None, None), scale=SCALE):
    return mod.bwd(do, q, k, v, out, lse, bufs[0], bufs[1], bufs[2], None, 0.0, scale, causal, window[0], window[1], 0.0, False, None, None)[:3]


def _assert_dv_kernel(be, bf16=None):
    s = be.last_schedule()
    assert s["fwd_kernel"] == 6 and s["d"] == D and s["dv"] == DV and s["name"].startswith("fa::fa_fwd_dv_kernel<"), s
    assert be.FWD_KERNEL_NAMES[s["fwd_kernel"]] == "fa_fwd_dv_kernel"
    if bf16 is not None:
        assert s["name"].startswith("fa::fa_fwd_dv_kernel<%s,192,128," % ("bf16" if bf16 else "f16")), s


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mode", ["full", "causal", "local"])
@pytest.mark.parametrize("sq,sk,h,hk", [(113, 203, 4, 4), (256, 512, 6, 2), (1024, 1024, 2, 1), (1, 300, 4, 2), (384, 129, 4, 4)])
def test_fwd_bwd_vs_fp32_reference(be, sq, sk, h, hk, mode, dtype):
    torch.manual_seed(0)
    B = 2
    q = torch.randn(B, sq, h, D, device="cuda", dtype=dtype)
    k = torch.randn(B, sk, hk, D, device="cuda", dtype=dtype)
    v = torch.randn(B, sk, hk, DV, device="cuda", dtype=dtype)
    do = torch.randn(B, sq, h, DV, device="cuda", dtype=dtype)
    causal = mode == "causal"
    window = (37, 50) if mode == "local" else (-1, -1)
    out, lse = _fwd(be, q, k, v, causal, window)
    _assert_dv_kernel(be, dtype == torch.bfloat16)
    assert out.shape == (B, sq, h, DV) and lse.shape == (B, h, sq)
    dq, dk, dv = _bwd(be, do, q, k, v, out, lse, causal, window)
    s = be.last_schedule()
    assert s["bwd_dq_nw"] == 4 and s["bwd_dkdv_nw"] == 4 and s["bwd_spill"] == 0, s   # never the 64-per-wave kernels or the fused modes
    _check(out, lse, (dq, dk, dv), q, k, v, do, causal, window)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sq", [1, 5, 300])
def test_one_hot_probabilities_give_v_rows_exactly(be, sq, dtype):
    """Every key row has two entries of 16.0 at its own pair of the 192 columns, every query row equals one key row, softmax_scale = 1: the
    chosen key scores 512, any other at most 256, so P is exactly one-hot -- out must be the chosen V rows bit for bit and lse 512.  A wrong V
    column map, a dropped k-step or a wrong tile offset shows exactly."""
    g = torch.Generator().manual_seed(5)
    B, Sk, H, Hk = 2, 1024, 8, 2
    pairs = torch.combinations(torch.arange(D), 2)                      # all C(192, 2) column pairs
    assert pairs.shape[0] == D * (D - 1) // 2
    k = torch.zeros(B, Sk, Hk, D)
    for b in range(B):
        for hk in range(Hk):
            sel = pairs[torch.randperm(pairs.shape[0], generator=g)[:Sk]]
            k[b, :, hk].scatter_(1, sel, 16.0)
    assert (k.sum(-1) == 32).all() and {int(c) for c in k.sum((0, 1, 2)).nonzero().flatten()} == set(range(D))   # every column = every k-step matters
    pick = torch.randint(0, Sk, (B, sq, H), generator=g)
    hk_of = torch.arange(H) // (H // Hk)
    q = k[torch.arange(B)[:, None, None], pick, hk_of[None, None, :]]   # (B, sq, H, D)
    v = torch.randn(B, Sk, Hk, DV, generator=g)
    v[v == 0] = 1.0
    q, k, v = (t.to("cuda", dtype) for t in (q, k, v))
    assert (v != 0).all()
    out, lse = _fwd(be, q, k, v, scale=1.0)
    _assert_dv_kernel(be)
    want = v[torch.arange(B, device="cuda")[:, None, None], pick.cuda(), hk_of.cuda()[None, None, :]]
    assert torch.equal(out, want)
    torch.testing.assert_close(lse, torch.full_like(lse, 512.0), rtol=2e-6, atol=0)


def _guard(shape, width, fill, dtype=torch.bfloat16, data=None):
    """A (..., shape[-1]) view of a (..., width) buffer whose other columns hold `fill`."""
    base = torch.full(shape[:-1] + (width,), fill, device="cuda", dtype=dtype)
    view = base[..., :shape[-1]]
    if data is not None:
        view.copy_(data)
    return base, view


@pytest.mark.parametrize("causal", [False, True])
def test_value_side_is_used_in_place(be, causal):
    """No padded or gathered copies: v, out, dout and dv are [..., :128] views of 192-wide buffers -- NaN behind the inputs' 128 columns, a
    sentinel in the outputs.  Results are finite, bitwise those of the call on contiguous tensors, and the sentinel columns stay untouched."""
    torch.manual_seed(1)
    B, sq, sk, h, hk = 2, 200, 333, 4, 2
    dt = torch.bfloat16
    q = torch.randn(B, sq, h, D, device="cuda", dtype=dt)
    k = torch.randn(B, sk, hk, D, device="cuda", dtype=dt)
    vc = torch.randn(B, sk, hk, DV, device="cuda", dtype=dt)
    doc = torch.randn(B, sq, h, DV, device="cuda", dtype=dt)
    _, v = _guard(vc.shape, D, float("nan"), data=vc)
    _, do = _guard(doc.shape, D, float("nan"), data=doc)
    SENT = 777.0
    ob, out_ = _guard((B, sq, h, DV), D, SENT)
    out, lse = _fwd(be, q, k, v, causal, out_=out_)
    _assert_dv_kernel(be)
    assert out.data_ptr() == out_.data_ptr() and torch.isfinite(out).all() and torch.isfinite(lse).all() and (ob[..., DV:] == SENT).all()
    oc, lc = _fwd(be, q, k, vc, causal)
    assert torch.equal(out, oc) and torch.equal(lse, lc)
    # backward: out behind NaN too (a fresh guarded copy), gradients into sentinel-guarded buffers
    _, og = _guard(oc.shape, D, float("nan"), data=oc)
    dqb, dq = _guard(q.shape, D + 32, SENT)
    dkb, dk = _guard(k.shape, D + 32, SENT)
    dvb, dv = _guard(vc.shape, D, SENT)
    _bwd(be, do, q, k, v, og, lse, causal, bufs=(dq, dk, dv))
    for base, view, w in ((dqb, dq, D), (dkb, dk, D), (dvb, dv, DV)):
        assert torch.isfinite(view).all() and (base[..., w:] == SENT).all()
    c = _bwd(be, doc, q, k, vc, oc, lc, causal)
    assert torch.equal(dq, c[0]) and torch.equal(dk, c[1]) and torch.equal(dv, c[2])
    assert c[2].shape == vc.shape


LENS = [0, 1, 129, 300, 1024]


def _packed(lens_q, lens_k, H, Hk, dtype=torch.bfloat16):
    cq = torch.tensor([0] + list(np.cumsum(lens_q)), dtype=torch.int32, device="cuda")
    ck = torch.tensor([0] + list(np.cumsum(lens_k)), dtype=torch.int32, device="cuda")
    q = torch.randn(sum(lens_q), H, D, device="cuda", dtype=dtype)
    k = torch.randn(sum(lens_k), Hk, D, device="cuda", dtype=dtype)
    v = torch.randn(sum(lens_k), Hk, DV, device="cuda", dtype=dtype)
    do = torch.randn(sum(lens_q), H, DV, device="cuda", dtype=dtype)
    return cq, ck, q, k, v, do


@pytest.mark.parametrize("causal", [False, True])
def test_varlen_parity_per_sequence(be, causal):
    torch.manual_seed(2)
    H, Hk = 6, 2
    cq, ck, q, k, v, do = _packed(LENS, LENS, H, Hk)
    out, lse = be.varlen_fwd(q, k, v, None, cq, ck, None, None, None, None, max(LENS), max(LENS), 0.0, SCALE, False, causal, -1, -1, 0.0,
                             False, None)[:2]
    _assert_dv_kernel(be)
    assert be.last_schedule()["fwd_list"] == 1
    assert out.shape == (sum(LENS), H, DV) and lse.shape == (H, sum(LENS))
    dq, dk, dv, _ = be.varlen_bwd(do, q, k, v, out, lse, None, None, None, cq, ck, None, max(LENS), max(LENS), 0.0, SCALE, False, causal,
                                  -1, -1, 0.0, False, None, None)
    assert dv.shape == v.shape
    for b, n in enumerate(LENS):
        if n == 0:
            continue
        qs, ks = slice(int(cq[b]), int(cq[b + 1])), slice(int(ck[b]), int(ck[b + 1]))
        _check(out[qs][None], lse[:, qs][None], (dq[qs][None], dk[ks][None], dv[ks][None]), q[qs][None], k[ks][None], v[ks][None], do[qs][None],
               causal, (-1, -1), what=f"seq {b} (len {n})")


def test_varlen_seqused_rows_past_them_are_not_written(be):
    """seqused_q / seqused_k shorten two entries: parity on the shortened sequences, and rows past them keep the sentinel (zero_tensors=False)."""
    torch.manual_seed(3)
    H, Hk = 6, 2
    cq, ck, q, k, v, do = _packed(LENS, LENS, H, Hk)
    used_q, used_k = [0, 1, 100, 300, 1024], [0, 1, 129, 257, 1024]     # entry 2 and entry 3 shortened
    uq = torch.tensor(used_q, dtype=torch.int32, device="cuda")
    uk = torch.tensor(used_k, dtype=torch.int32, device="cuda")
    SENT = 777.0
    out_ = torch.full((sum(LENS), H, DV), SENT, device="cuda", dtype=q.dtype)
    out, lse = be.varlen_fwd(q, k, v, out_, cq, ck, uk, None, None, None, max(LENS), max(LENS), 0.0, SCALE, False, True, -1, -1, 0.0,
                             False, None, 0, seqused_q=uq)[:2]
    _assert_dv_kernel(be)
    dq_, dk_, dv_ = (torch.full_like(t, SENT) for t in (q, k, v))
    dq, dk, dv, _ = be.varlen_bwd(do, q, k, v, out, lse, dq_, dk_, dv_, cq, ck, None, max(LENS), max(LENS), 0.0, SCALE, False, True, -1, -1,
                                  0.0, False, None, None, seqused_q=uq, seqused_k=uk)
    for b, n in enumerate(LENS):
        q0, k0 = int(cq[b]), int(ck[b])
        nq, nk = used_q[b], used_k[b]
        assert (out[q0 + nq:q0 + n] == SENT).all() and (dq[q0 + nq:q0 + n] == SENT).all()
        assert (dk[k0 + nk:k0 + n] == SENT).all() and (dv[k0 + nk:k0 + n] == SENT).all()
        if nq == 0:
            continue
        qs, ks = slice(q0, q0 + nq), slice(k0, k0 + nk)
        _check(out[qs][None], lse[:, qs][None], (dq[qs][None], dk[ks][None], dv[ks][None]), q[qs][None], k[ks][None], v[ks][None], do[qs][None],
               True, (-1, -1), what=f"seq {b} (used {nq}/{nk})")


def test_gqa_group_split_backward(be):
    """B = 2, S = 1024, H = 32, Hk = 2, causal: 16 key-block workgroups would not fill the chip, the dK/dV kernel splits the GQA group into virtual
    kv heads and sums the partials -- dK's at width 192, dV's at width 128.  Parity, and bitwise equal results on a second run."""
    from flash_attn_amd import _cabi
    torch.manual_seed(4)
    B, S, H, Hk = 2, 1024, 32, 2
    q = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, S, Hk, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, S, Hk, DV, device="cuda", dtype=torch.bfloat16)
    do = torch.randn(B, S, H, DV, device="cuda", dtype=torch.bfloat16)
    a = _cabi.FaBwdParams()
    a.b, a.h, a.h_k, a.d, a.d_v, a.seqlen_q, a.seqlen_k, a.dtype, a.is_causal = B, H, Hk, D, DV, S, S, _cabi.FA_DTYPE_BF16, 1
    plan = (C.c_int32 * 8)()
    assert _cabi.load().fa_bwd_plan_query(C.byref(a), plan, 8) == 8 and plan[0] == 0 and plan[3] >= 2, list(plan)   # the pair, group split
    out, lse = _fwd(be, q, k, v, True)
    g1 = _bwd(be, do, q, k, v, out, lse, True)
    g2 = _bwd(be, do, q, k, v, out, lse, True)
    assert g1[2].shape == (B, S, Hk, DV)
    for x, y in zip(g1, g2):
        assert torch.equal(x, y)
    _check(out, lse, g1, q, k, v, do, True, (-1, -1))


def test_binders_agree_bit_for_bit(be):
    ext = pytest.importorskip("flash_attn_2_cuda")
    torch.manual_seed(6)
    B, sq, sk, H, Hk = 2, 200, 333, 4, 2
    q = torch.randn(B, sq, H, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, sk, Hk, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, sk, Hk, DV, device="cuda", dtype=torch.bfloat16)
    do = torch.randn(B, sq, H, DV, device="cuda", dtype=torch.bfloat16)
    o1, l1 = _fwd(be, q, k, v, True)
    o2, l2 = _fwd(ext, q, k, v, True)
    _assert_dv_kernel(be)
    assert o2.shape == (B, sq, H, DV) and torch.equal(o1, o2) and torch.equal(l1, l2)
    for x, y in zip(_bwd(be, do, q, k, v, o1, l1, True), _bwd(ext, do, q, k, v, o2, l2, True)):
        assert x.shape == y.shape and torch.equal(x, y)
    lens_q, lens_k = [70, 1, 200, 33], [90, 64, 200, 257]
    cq, ck, q, k, v, do = _packed(lens_q, lens_k, H, Hk)
    r = []
    for mod in (be, ext):
        o, l = mod.varlen_fwd(q, k, v, None, cq, ck, None, None, None, None, max(lens_q), max(lens_k), 0.0, SCALE, False, True, -1, -1, 0.0,
                              False, None)[:2]
        g = mod.varlen_bwd(do, q, k, v, o, l, None, None, None, cq, ck, None, max(lens_q), max(lens_k), 0.0, SCALE, False, True, -1, -1, 0.0,
                           False, None, None)[:3]
        r.append((o, l) + tuple(g))
    for x, y in zip(*r):
        assert x.shape == y.shape and torch.equal(x, y)
    # the refusals reach the extension's callers as RuntimeError naming both head dims
    with pytest.raises(RuntimeError, match=r"192.*96"):
        _fwd(ext, q[None], k[None], v[None, ..., :96].contiguous())
    with pytest.raises(RuntimeError, match=r"192.*128.*softcap"):
        ext.fwd(q[None], k[None], v[None], None, None, 0.0, SCALE, False, -1, -1, 30.0, False, None)


def test_public_api_autograd_default_scale_and_export(be):
    from flash_attn_amd import flash_attn_interface as fi
    torch.manual_seed(7)
    B, sq, sk, H, Hk = 2, 150, 260, 4, 2
    q = torch.randn(B, sq, H, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(B, sk, Hk, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(B, sk, Hk, DV, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    out = fi.flash_attn_func(q, k, v, causal=True)
    _assert_dv_kernel(be)
    assert out.shape == (B, sq, H, DV)
    o_b, l_b = _fwd(be, q.detach(), k.detach(), v.detach(), True, scale=192 ** -0.5)   # the default scale is q's head dim ** -0.5
    assert torch.equal(out, o_b)
    out.sum().backward()
    gb = _bwd(be, torch.ones_like(o_b), q.detach(), k.detach(), v.detach(), o_b, l_b, True)
    for t, g in zip((q, k, v), gb):
        assert t.grad.shape == t.shape and torch.equal(t.grad, g)
    # packed batch through the public function
    lens = [70, 1, 200, 33]
    cq, ck, qp, kp, vp, do = _packed(lens, lens, H, Hk)
    qp, kp, vp = (t.requires_grad_() for t in (qp, kp, vp))
    op = fi.flash_attn_varlen_func(qp, kp, vp, cq, ck, max(lens), max(lens), causal=True)
    assert op.shape == (sum(lens), H, DV)
    op.backward(do)
    assert qp.grad.shape == qp.shape and kp.grad.shape == kp.shape and vp.grad.shape == vp.shape
    ob, lb = be.varlen_fwd(qp.detach(), kp.detach(), vp.detach(), None, cq, ck, None, None, None, None, max(lens), max(lens), 0.0, SCALE, False,
                           True, -1, -1, 0.0, False, None)[:2]
    gv = be.varlen_bwd(do, qp.detach(), kp.detach(), vp.detach(), ob, lb, None, None, None, cq, ck, None, max(lens), max(lens), 0.0, SCALE, False,
                       True, -1, -1, 0.0, False, None, None)[:3]
    assert torch.equal(op, ob) and all(torch.equal(t.grad, g) for t, g in zip((qp, kp, vp), gv))

    # an exported program holds the raw op; it still differentiates (the op's registered autograd formula)
    class M(torch.nn.Module):
        def forward(self, q, k, v):
            return torch.ops.flash_attn_amd._flash_attn_forward(q, k, v, 0.0, SCALE, True, -1, -1, 0.0, None, False)[0]

    qd, kd, vd = (t.detach().clone().requires_grad_() for t in (q, k, v))
    ep = torch.export.export(M(), (qd, kd, vd))
    assert any("flash_attn_amd" in str(n.target) for n in ep.graph.nodes)
    got = ep.module()(qd, kd, vd)
    assert got.shape == (B, sq, H, DV) and torch.equal(got, o_b)
    got.sum().backward()
    for t, g in zip((qd, kd, vd), gb):
        assert torch.equal(t.grad, g)


@pytest.mark.parametrize("d", [192, 128])
def test_equal_head_dims_keep_their_kernels(be, d):
    """D = Dv calls are untouched: the kernels and names they had."""
    torch.manual_seed(8)
    q = torch.randn(2, 256, 4, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(2, 256, 2, d, device="cuda", dtype=torch.bfloat16)
    v = torch.randn_like(k)
    out, lse = _fwd(be, q, k, v, True, scale=d ** -0.5)
    s = be.last_schedule()
    assert s["fwd_kernel"] in (1, 2, 3) and s["d"] == d and s["dv"] == d, s
    if d == 192:
        assert s["name"] == "fa::fa_fwd_kernel<bf16,192,4,feat0,lockstep>", s
    else:
        assert s["name"].startswith("fa::fa_fwd_il_kernel<bf16,128,") or s["name"].startswith("fa::fa_fwd_w64_kernel<"), s
    o32, _ = attention_torch(q.float(), k.float(), v.float(), True)
    opt, _ = attention_torch(q, k, v, True, upcast=False, reorder=True)
    assert max_abs(out.float(), o32) <= 2 * max_abs(opt.float(), o32) + 1e-4
