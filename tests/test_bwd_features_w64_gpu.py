"""Softcap and dropout on the 64-rows-per-wave dQ kernel (csrc/fa_bwd_w64.hip: fa_bwd_dq_w64_kernel<.., FEAT_CAP / FEAT_DROP>, round 5; reference: the
Is_softcap / Is_dropout switches of the one backward kernel, csrc/flash_attn/src/flash_bwd_kernel.h:457-733, utils.h:395-409, dropout.h).  dK / dV of these
features stay on the eight-wave kernel of fa_bwd.hip, so the knob FA_BWD_DQ_NW decides dQ alone: 64 against 4 (the established feature kernel) on the same
inputs and the same forward.  dQ must
  * sit inside the reference suite's rule against an fp32 PyTorch evaluation of the same attention (error <= 3x the error of PyTorch in the input dtype; for
    dropout the mask comes from the forward's return_softmax payload), and within 4x the established kernel's error (the 64-rows kernel multiplies by a Q that
    was scaled and rounded once, the established one scales every score in fp32),
  * be bitwise reproducible; dK / dV must not move at all when only the dQ kernel changes -- except through softmax_d, which the 64-rows kernel computes itself
    in another summation order (compared with a tolerance)."""
import pytest
import torch

from tests._dropout_model import threshold as dropout_threshold

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from flash_attn_amd import backend
    return backend


def torch_grads(q, k, v, do, causal, wl, wr, softcap, keep, p, exact):
    """Gradients of attention with softcap / a given dropout mask; exact: fp32 math, else products and P in the input dtype."""
    qf, kf, vf = [(x.float() if exact else x).transpose(1, 2).detach().requires_grad_(True) for x in (q, k, v)]
    g = qf.shape[1] // kf.shape[1]
    s = (qf @ (kf * q.shape[-1] ** -0.5).repeat_interleave(g, 1).transpose(-1, -2)).float()
    if softcap > 0:
        s = softcap * torch.tanh(s / softcap)
    Sq, Sk = s.shape[-2:]
    i = torch.arange(Sq, device=q.device)[:, None] + (Sk - Sq)
    j = torch.arange(Sk, device=q.device)[None]
    m = torch.zeros(Sq, Sk, dtype=torch.bool, device=q.device)
    if causal:
        wr = 0
    if wr >= 0:
        m |= j > i + wr
    if wl >= 0:
        m |= j < i - wl
    pr = torch.softmax(s.masked_fill(m, float("-inf")), -1).nan_to_num(0.0)
    if keep is not None:
        pr = pr * keep.float() / (1.0 - p)
    pr = pr if exact else pr.to(q.dtype)
    (pr @ vf.repeat_interleave(g, 1)).backward((do.float() if exact else do).transpose(1, 2))
    return [x.grad.transpose(1, 2) for x in (qf, kf, vf)]


SHAPES = [  # B, Sq, Sk, H, Hk, causal, wl, wr
    (2, 512, 512, 4, 4, True, -1, -1), (1, 1024, 1024, 4, 2, False, -1, -1), (2, 333, 777, 6, 2, True, -1, -1), (1, 2048, 2048, 4, 2, True, 256, 0),
    (1, 777, 333, 4, 4, True, -1, -1), (1, 65, 513, 2, 1, False, -1, -1), (1, 200, 200, 2, 2, False, 64, 32), (1, 31, 31, 1, 1, True, -1, -1),
    (1, 1, 700, 2, 2, False, -1, -1), (1, 700, 1, 2, 1, True, -1, -1), (1, 1500, 1500, 2, 1, False, -1, 0),
]


@pytest.mark.parametrize("d", [128])   # (head dim 64 keeps the 4-wave feature kernel: the 64-rows variants measured 2-4 % behind it there and are not built)
@pytest.mark.parametrize("feature,dtype", [("softcap", torch.bfloat16), ("softcap", torch.float16), ("dropout", torch.bfloat16), ("dropout", torch.float16)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_Sq%d_Sk%d_H%d_%d_c%d_w%d_%d" % s)
def test_dq_w64_softcap_and_dropout(be, knobs, shape, feature, dtype, d):
    B, Sq, Sk, H, Hk, causal, wl, wr = shape
    torch.manual_seed(0)
    q = torch.randn(B, Sq, H, d, device="cuda", dtype=dtype)
    k = torch.randn(B, Sk, Hk, d, device="cuda", dtype=dtype)
    v, do = torch.randn_like(k), torch.randn_like(q)
    cap, p = (25.0, 0.0) if feature == "softcap" else (0.0, 0.2)
    sc = d ** -0.5
    torch.manual_seed(21)
    out, lse, rv, rng = be.fwd(q, k, v, None, None, p, sc, causal, wl, wr, cap, p > 0, None)
    keep = (rv.to(torch.int32) <= dropout_threshold(p)) if p > 0 else None
    bwd = lambda: be.bwd(do, q, k, v, out, lse, None, None, None, None, p, sc, causal, wl, wr, cap, False, None, rng)
    knobs.set("FA_BWD_DQ_NW", 4)
    g_old = bwd()
    assert be.last_schedule()["bwd_dq_nw"] == 4
    knobs.set("FA_BWD_DQ_NW", 64)
    g_new = bwd()
    assert be.last_schedule()["bwd_dq_nw"] == 64, be.last_schedule()
    again = bwd()
    assert all(torch.equal(a, b) for a, b in zip(g_new[:3], again[:3])), "run-to-run"
    assert torch.equal(g_old[2], g_new[2]), "dV does not see the dQ kernel"
    assert float((g_old[1].float() - g_new[1].float()).abs().max()) <= 2e-2 * max(1.0, float(g_old[1].float().abs().max())), "dK moves only through softmax_d's rounding"
    r = torch_grads(q, k, v, do, causal, wl, wr, cap, keep, p, True)
    pt = torch_grads(q, k, v, do, causal, wl, wr, cap, keep, p, False)
    floor = (1e-2 if dtype == torch.bfloat16 else 2e-3) / (1.0 - p)
    assert torch.isfinite(g_new[0].float()).all()
    e_old, e_new, e_pt = [float((x[0].float() - r[0]).abs().max()) for x in (g_old, g_new, pt)]
    assert e_new <= max(3 * e_pt, floor), (e_new, e_pt)
    assert e_new <= max(4 * e_old, floor), (e_new, e_old)


@pytest.mark.parametrize("feature", ["softcap", "dropout"])
def test_dq_w64_features_packed_batch(be, knobs, feature):
    """Through varlen_bwd: the packed batch against the 4-wave feature kernel on the same packed batch (dropout: each sequence's rows and keys count from 0 in the
    random stream in both kernels)."""
    import itertools
    torch.manual_seed(3)
    lens_q = [700, 33, 1500, 256, 64, 1, 900, 0, 300]
    lens_k = [700, 65, 1500, 300, 64, 77, 513, 5, 1]
    H, Hk, d = 4, 2, 128
    cu_q = torch.tensor([0] + list(itertools.accumulate(lens_q)), dtype=torch.int32, device="cuda")
    cu_k = torch.tensor([0] + list(itertools.accumulate(lens_k)), dtype=torch.int32, device="cuda")
    q = torch.randn(sum(lens_q), H, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(sum(lens_k), Hk, d, device="cuda", dtype=torch.bfloat16)
    v, do = torch.randn_like(k), torch.randn_like(q)
    cap, p = (25.0, 0.0) if feature == "softcap" else (0.0, 0.2)
    sc = d ** -0.5
    torch.manual_seed(5)
    out, lse, _, rng = be.varlen_fwd(q, k, v, None, cu_q, cu_k, None, None, None, None, max(lens_q), max(lens_k), p, sc, False, True, -1, -1, cap, False, None)
    bwd = lambda: be.varlen_bwd(do, q, k, v, out, lse, None, None, None, cu_q, cu_k, None, max(lens_q), max(lens_k), p, sc, False, True, -1, -1, cap, False, None, rng)[:3]
    knobs.set("FA_BWD_DQ_NW", 4)
    a = bwd()
    knobs.set("FA_BWD_DQ_NW", 64)
    w = bwd()
    assert be.last_schedule()["bwd_dq_nw"] == 64
    assert torch.isfinite(w[0].float()).all()
    assert float((a[0].float() - w[0].float()).abs().max()) <= 4e-2 * max(1.0, float(a[0].float().abs().max()))
    assert torch.equal(a[2], w[2])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES + [(1, 4096, 4096, 2, 2, True, -1, -1), (1, 3000, 3000, 4, 1, True, 1024, 0)], ids=lambda s: "B%d_Sq%d_Sk%d_H%d_%d_c%d_w%d_%d" % s)
def test_dkdv_w64_softcap(be, knobs, shape, dtype):
    """Softcap on the 64-keys-per-wave dK/dV kernel (fa_bwd_dkdv_w64_kernel<.., FEAT_CAP>, head dim 128): the chains start from C = 0, the rows' c - LSE*log2e are
    read in phase B, the cap and its derivative take three staged gaps per element.  FA_BWD_DKDV = 64 against 8 (the eight-wave feature kernel) with the dQ kernel
    held fixed: dK / dV under the 3x-PyTorch rule and within 2x the eight-wave kernel's error (both scale every score in fp32), bitwise run-to-run, dQ untouched."""
    B, Sq, Sk, H, Hk, causal, wl, wr = shape
    d, cap = 128, 25.0
    torch.manual_seed(0)
    q = torch.randn(B, Sq, H, d, device="cuda", dtype=dtype)
    k = torch.randn(B, Sk, Hk, d, device="cuda", dtype=dtype)
    v, do = torch.randn_like(k), torch.randn_like(q)
    sc = d ** -0.5
    out, lse, _, _ = be.fwd(q, k, v, None, None, 0.0, sc, causal, wl, wr, cap, False, None)
    bwd = lambda: be.bwd(do, q, k, v, out, lse, None, None, None, None, 0.0, sc, causal, wl, wr, cap, False, None, None)
    knobs.set("FA_BWD_DQ_NW", 4)
    knobs.set("FA_BWD_DKDV", 8)
    g8 = bwd()
    assert be.last_schedule()["bwd_dkdv_nw"] == 8
    knobs.set("FA_BWD_DKDV", 64)
    g64 = bwd()
    assert be.last_schedule()["bwd_dkdv_nw"] == 64, be.last_schedule()
    again = bwd()
    assert all(torch.equal(a, b) for a, b in zip(g64[:3], again[:3])), "run-to-run"
    assert torch.equal(g8[0], g64[0]), "dQ is not this kernel's"
    r = torch_grads(q, k, v, do, causal, wl, wr, cap, None, 0.0, True)
    pt = torch_grads(q, k, v, do, causal, wl, wr, cap, None, 0.0, False)
    floor = 1e-2 if dtype == torch.bfloat16 else 2e-3
    for i, name in ((1, "dk"), (2, "dv")):
        assert torch.isfinite(g64[i].float()).all(), name
        e8, e64, e_pt = [float((x[i].float() - r[i]).abs().max()) for x in (g8, g64, pt)]
        assert e64 <= max(3 * e_pt, floor), (name, e64, e_pt)
        assert e64 <= max(2 * e8, floor), (name, e64, e8)
