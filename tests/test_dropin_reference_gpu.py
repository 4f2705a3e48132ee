"""The literal drop-in: the REFERENCE's Python package (flash_attn/flash_attn_interface.py, its torch.library custom ops
flash_attn::_flash_attn_forward / _backward / ..., :84-458) importing OUR module `flash_attn_2_cuda`, forward + backward
against the fp64 oracle.  The reference tree is not part of this repository and does not exist on the driver's GPU box:
the test runs only when $FLASH_ATTN_REF names a readable tree (opt-in: it executes third-party code; recorded runs: profiles/r02_dropin_reference.txt,
profiles/r04_reference_suite.txt) and SKIPS -- saying so -- otherwise.  No copy of that tree is made or shipped anywhere by this repository's tools."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "flash-attention_amd")


def _reference_root():
    # Opt-in only: these tests import and EXECUTE a third-party package.  Nothing is auto-discovered; the caller names the tree
    # (FLASH_ATTN_REF=<a checkout of the reference>, on a machine that has one).
    cand = os.environ.get("FLASH_ATTN_REF")
    if cand and os.path.exists(os.path.join(cand, "flash_attn", "flash_attn_interface.py")):
        return cand
    return None


@pytest.fixture(scope="module")
def ref_flash_attn():
    root = _reference_root()
    if root is None:
        pytest.skip("reference flash_attn package not readable on this box (set FLASH_ATTN_REF): literal drop-in not exercised")
    for p in (root, PKG):      # ours first: `import flash_attn_2_cuda` must resolve to the gfx950 extension
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)
    for m in [m for m in sys.modules if m == "flash_attn" or m.startswith("flash_attn.")]:
        del sys.modules[m]
    fa = importlib.import_module("flash_attn")
    import flash_attn_2_cuda as ext
    assert os.path.dirname(ext.__file__) == PKG, ext.__file__
    assert os.path.realpath(fa.__file__).startswith(os.path.realpath(root)), fa.__file__
    iface = importlib.import_module("flash_attn.flash_attn_interface")
    assert iface.flash_attn_gpu is ext
    return fa


def _close(got, ref, tol):
    return float((got.detach().float().cpu() - torch.from_numpy(np.asarray(ref)).float()).abs().max()) < tol


@pytest.mark.parametrize("causal", [False, True])
def test_reference_flash_attn_func_on_our_backend(ref_flash_attn, causal):
    from oracle import attention_oracle as orc
    torch.manual_seed(0)
    q = torch.randn(2, 300, 8, 128, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(2, 333, 2, 128, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(2, 333, 2, 128, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    out = ref_flash_attn.flash_attn_func(q, k, v, causal=causal)
    g = torch.randn_like(out)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), g)
    o_ref, _ = orc.attention_fwd(q, k, v, None, causal)
    gr = orc.attention_bwd(g, q, k, v, None, None, None, causal)
    assert _close(out, o_ref, 2e-2) and _close(dq, gr[0], 6e-2) and _close(dk, gr[1], 6e-2) and _close(dv, gr[2], 6e-2)


def test_reference_varlen_and_packed_funcs_on_our_backend(ref_flash_attn):
    from oracle import attention_oracle as orc
    torch.manual_seed(1)
    lens = [64, 1, 200, 129]
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda")
    qkv = torch.randn(sum(lens), 3, 4, 64, device="cuda", dtype=torch.float16, requires_grad=True)
    out = ref_flash_attn.flash_attn_varlen_qkvpacked_func(qkv, cu, max(lens), causal=True)
    g = torch.randn_like(out)
    (dqkv,) = torch.autograd.grad(out, (qkv,), g)
    q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]
    o_ref, _ = orc.varlen_fwd(q, k, v, cu.cpu().numpy(), cu.cpu().numpy(), None, True)
    gr = orc.varlen_bwd(g, q, k, v, cu.cpu().numpy(), cu.cpu().numpy(), None, True)
    assert _close(out, o_ref, 1e-2)
    for i in range(3):
        assert _close(dqkv[:, i], gr[i], 4e-2), i


def test_reference_flash_attn_with_kvcache_on_our_backend(ref_flash_attn):
    from oracle import attention_oracle as orc
    torch.manual_seed(2)
    B, H, Hk, D, S = 3, 8, 2, 128, 1024
    q = torch.randn(B, 1, H, D, device="cuda", dtype=torch.bfloat16)
    kc = torch.randn(B, S, Hk, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    kn = torch.randn(B, 1, Hk, D, device="cuda", dtype=torch.bfloat16)
    vn = torch.randn_like(kn)
    lens = torch.tensor([100, 517, 1023], dtype=torch.int32, device="cuda")
    kc0, vc0 = kc.clone(), vc.clone()
    out = ref_flash_attn.flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=lens, causal=True)
    for b in range(B):
        n = int(lens[b])
        kk = torch.cat([kc0[b:b + 1, :n], kn[b:b + 1]], 1)
        vv = torch.cat([vc0[b:b + 1, :n], vn[b:b + 1]], 1)
        o_ref, _ = orc.attention_fwd(q[b:b + 1], kk, vv, None, False)
        assert _close(out[b:b + 1], o_ref, 2e-2), b
        assert torch.equal(kc[b, n], kn[b, 0]) and torch.equal(vc[b, n], vn[b, 0])


def test_reference_mha_modules_on_our_backend(ref_flash_attn):
    """The reference's own attention modules (flash_attn/modules/mha.py:53-131 FlashSelfAttention -- packed QKV, fixed and cu_seqlens, dropout in
    training -- and :133-225 FlashCrossAttention -- q + packed KV) imported from the reference tree, running on the in-tree backend module."""
    from oracle import attention_oracle as orc
    from flash_attn.modules.mha import FlashCrossAttention, FlashSelfAttention
    torch.manual_seed(3)
    B, S, H, D = 2, 257, 4, 64
    qkv = torch.randn(B, S, 3, H, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    sa = FlashSelfAttention(causal=True, attention_dropout=0.0).cuda()
    out = sa(qkv)
    g = torch.randn_like(out)
    (dqkv,) = torch.autograd.grad(out, qkv, g)
    q, k, v = qkv.unbind(2)
    o_ref, _ = orc.attention_fwd(q, k, v, None, True)
    gr = orc.attention_bwd(g, q, k, v, None, None, None, True)
    assert _close(out, o_ref, 2e-2)
    for i in range(3):
        assert _close(dqkv[:, :, i], gr[i], 6e-2), i
    # cu_seqlens form
    lens = [100, 1, 156]
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda")
    qkv_p = torch.randn(sum(lens), 3, H, D, device="cuda", dtype=torch.bfloat16)
    out_p = sa(qkv_p, cu_seqlens=cu, max_seqlen=max(lens))
    o_ref, _ = orc.varlen_fwd(qkv_p[:, 0], qkv_p[:, 1], qkv_p[:, 2], cu.cpu().numpy(), cu.cpu().numpy(), None, True)
    assert _close(out_p, o_ref, 2e-2)
    # dropout in training mode runs (mask statistics are tested through our own interface, tests/test_dropout_gpu.py)
    sa_d = FlashSelfAttention(causal=False, attention_dropout=0.2).cuda().train()
    out_d = sa_d(qkv)
    assert out_d.shape == out.shape and torch.isfinite(out_d.float()).all()
    # cross attention: q (B,Sq,H,D) + kv (B,Sk,2,Hk,D)
    ca = FlashCrossAttention(causal=False).cuda()
    qx = torch.randn(B, 77, H, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    kv = torch.randn(B, 300, 2, H, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    ox = ca(qx, kv)
    gx = torch.randn_like(ox)
    dqx, dkv = torch.autograd.grad(ox, (qx, kv), gx)
    o_ref, _ = orc.attention_fwd(qx, kv[:, :, 0], kv[:, :, 1], None, False)
    gr = orc.attention_bwd(gx, qx, kv[:, :, 0], kv[:, :, 1], None, None, None, False)
    assert _close(ox, o_ref, 2e-2) and _close(dqx, gr[0], 6e-2) and _close(dkv[:, :, 0], gr[1], 6e-2) and _close(dkv[:, :, 1], gr[2], 6e-2)
