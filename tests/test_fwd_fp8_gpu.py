"""GPU suite of the FP8 (e4m3) forward (csrc/fa_fwd_fp8.hip through fa_fwd_fp8 / fa_varlen_fwd_fp8).

Inputs are built on the CPU and copied over; every reference is evaluated on the CPU.
  - one-hot: integer rows that make P exactly one-hot -- any error in the MFMA lane maps, the P^T packing or the V^T image picks the wrong row;
  - parity: FA3's rule (hopper/test_flash_attn.py:226-289) in our words -- |out - ref| <= 2 max|emu - ref| + 2 bf16-eps |ref|, ref = the
    fp64 oracle on dequantised inputs, emu = fp32 attention with the probabilities rounded to e4m3; the LSE within 5e-4 max(1, |LSE|) of it;
  - varlen against per-sequence calls, determinism, edge cases, binders, the public API and the two real shapes."""
import itertools
import zlib

import numpy as np
import pytest
import torch

from oracle import attention_oracle as orc

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn
DEV = "cuda"
BF16_EPS = 2.0 ** -8


def _be():
    from flash_attn_amd import backend
    return backend


def _fp8(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(FP8)   # test-input quantisation, on the CPU


def _descales(kind, B, Hk, g):
    """None, contiguous random (0, 2) or a non-contiguous (Hk, B)^T view, built on the device."""
    if kind is None:
        return None, None, None
    out = []
    for _ in range(3):
        if kind == "rand":
            out.append((torch.rand(B, Hk, generator=g) * 1.9 + 0.05).to(DEV))
        else:
            out.append((torch.rand(Hk, B, generator=g) * 1.9 + 0.05).to(DEV).t())
    return tuple(out)


def _dequant(x, ds, B, Hk):
    """(B, S, heads, D) fp8 -> float64 numpy times ds[b, head // (heads / Hk)]."""
    xf = x.to(torch.float64)
    if ds is None:
        return xf.numpy()
    g = x.shape[2] // Hk
    d = ds.detach().cpu().to(torch.float64).repeat_interleave(g, dim=1)   # (B, heads)
    return (xf * d[:, None, :, None]).numpy()


def _emulate(q, k, v, scale, causal, window):
    """fp32 attention on dequantised float64 inputs with the softmax probabilities rounded to e4m3 before the product with V -- the
    reference's `intermediate_dtype` (hopper/test_util.py:343-344)."""
    q, k, v = (torch.from_numpy(x).float() for x in (q, k, v))
    B, Sq, H, D = q.shape
    Sk, Hk = k.shape[1], k.shape[2]
    g = H // Hk
    k, v = k.repeat_interleave(g, dim=2), v.repeat_interleave(g, dim=2)
    s = torch.einsum("bthd,bshd->bhts", q, k) * scale
    _, wl, wr = orc.normalize_window(Sq, Sk, causal, window[0], window[1])
    vis = torch.from_numpy(orc.visible_mask(Sq, Sk, wl, wr))
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    p8 = (p / torch.where(l > 0, l, torch.ones_like(l))).to(FP8).float()
    o = torch.einsum("bhts,bshd->bthd", p8, v)
    return o.double().numpy()


def _run(q, k, v, ds, scale, causal, window, out_=None):
    be = _be()
    qd, kd, vd = ds
    return be.fwd_fp8(q.to(DEV), k.to(DEV), v.to(DEV), out_, qd, kd, vd, scale, causal, window[0], window[1])


def _check_parity(q, k, v, ds, scale, causal, window, out, lse, rows=None):
    """FA3's rule against the fp64 oracle; returns (max |out - ref|, max |lse - ref|)."""
    qd, kd, vd = ds
    if rows is not None:   # one (batch, head) unit of a large shape
        b, h = rows
        hk = h // (q.shape[2] // k.shape[2])
        q, k, v = q[b:b + 1, :, h:h + 1], k[b:b + 1, :, hk:hk + 1], v[b:b + 1, :, hk:hk + 1]
        qd, kd, vd = (None if t is None else t[b:b + 1, hk:hk + 1] for t in (qd, kd, vd))
        out, lse = out[b:b + 1, :, h:h + 1], lse[b:b + 1, h:h + 1]
    B, Hk = q.shape[0], k.shape[2]
    qf, kf, vf = _dequant(q, qd, B, Hk), _dequant(k, kd, B, Hk), _dequant(v, vd, B, Hk)
    ref_o, ref_l = orc.attention_fwd(qf, kf, vf, scale, causal, window)
    emu = _emulate(qf, kf, vf, scale, causal, window)
    o = out.detach().cpu().double().numpy()
    l = lse.detach().cpu().double().numpy()
    assert np.isfinite(o).all()
    tol = 2 * np.abs(emu - ref_o).max() + 2 * BF16_EPS * np.abs(ref_o) + 1e-6
    err_o = np.abs(o - ref_o)
    assert (err_o <= tol).all(), (float(err_o.max()), float(np.abs(emu - ref_o).max()))
    fin = np.isfinite(ref_l)
    assert (np.isfinite(l) == fin).all() and (l[~fin] == np.inf).all()
    # (measured on MI355X: the scaled MFMA's e4m3 dot products are not exact fp32 sums -- LSE errors up to 7.6e-4 absolute, 2.3e-4 relative
    # to max(1, |LSE|) over this grid, where exact sums would give ~1e-6 -- so the bound is relative, at twice the measured worst case)
    err_l = float((np.abs(l[fin] - ref_l[fin]) / np.maximum(1.0, np.abs(ref_l[fin]))).max()) if fin.any() else 0.0
    assert err_l < 5e-4, err_l
    return float(err_o.max()), err_l


# ---- exact one-hot probe (written first: a lane-map or key-permutation error shows as a wrong row, not as noise) -----------------------
@pytest.mark.parametrize("Sk", [64, 100, 128, 192])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_fp8_one_hot_rows_are_exact(Sk, D, causal):
    g = torch.Generator().manual_seed(1000 * Sk + D + causal)
    B, H, Hk, Sq = 2, 4, 2, Sk
    pairs = list(itertools.combinations(range(D), 2))
    sel = torch.randperm(len(pairs), generator=g)[:Sk]
    k = torch.zeros(B, Sk, Hk, D)
    for j, idx in enumerate(sel.tolist()):
        a, b = pairs[idx]
        k[:, j, :, a] = 16.0
        k[:, j, :, b] = 16.0
    shift = Sk - Sq
    tgt = torch.empty(B, Sq, H, dtype=torch.long)
    for i in range(Sq):
        hi = i + shift if causal else Sk - 1
        tgt[:, i, :] = torch.randint(0, hi + 1, (B, H), generator=g)
    q = torch.zeros(B, Sq, H, D)
    for b in range(B):
        for h in range(H):
            q[b, :, h] = k[b, tgt[b, :, h], h // (H // Hk)]
    # v without zeros: a rescale factor 2^-92 times an earlier row must not show up as a nonzero output element
    v = (torch.sign(torch.randn(B, Sk, Hk, D, generator=g)) * (0.5 + 3.5 * torch.rand(B, Sk, Hk, D, generator=g))).to(FP8)
    qd, kd, vd = ((torch.rand(B, Hk, generator=g) * 1.5 + 0.5) for _ in range(3))
    out, lse = _run(q.to(FP8), k.to(FP8), v, (qd.to(DEV), kd.to(DEV), vd.to(DEV)), 1.0, causal, (-1, -1))
    assert _be().last_schedule()["fwd_kernel"] == 4
    out, lse = out.cpu(), lse.cpu()
    g_ = H // Hk
    for b in range(B):
        for h in range(H):
            hk = h // g_
            want = (vd[b, hk] * v[b, tgt[b, :, h], hk].float()).to(torch.bfloat16)
            assert torch.equal(out[b, :, h], want), (b, h, (out[b, :, h].float() - want.float()).abs().max())
            want_l = torch.full((Sq,), 512.0) * qd[b, hk] * kd[b, hk]
            torch.testing.assert_close(lse[b, h], want_l, rtol=2e-6, atol=0)


# ---- parity grid ---------------------------------------------------------------------------------------------------------------------
_SEQS = [(1, 1), (113, 203), (128, 128), (512, 300), (1000, 1000), (2048, 2048)]
_HEADS = [(4, 4), (6, 2), (8, 1)]
_MASKS = [(False, (-1, -1)), (True, (-1, -1)), (False, (64, 0)), (False, (32, 16))]
_DKINDS = [None, "rand", "t"]


def _grid():
    """Every (Sq, Sk) x heads x D x mask for the short sequences; the two long ones at GQA 6/2.  Batch size and descale kind rotate over the cases."""
    out = []
    for (sq, sk), (h, hk), d, (causal, win) in itertools.product(_SEQS, _HEADS, (64, 128), _MASKS):
        if sq >= 1000 and (h, hk) != (6, 2):
            continue
        i = len(out)
        bb = 1 + (i + i // 4) % 2
        out.append(pytest.param(bb, sq, sk, h, hk, d, causal, win, _DKINDS[i % 3],
                                id=f"B{bb}-{sq}x{sk}-h{h}/{hk}-d{d}-{'causal' if causal else 'win%d_%d' % win}-{_DKINDS[i % 3]}"))
    return out


@pytest.mark.parametrize("B,Sq,Sk,H,Hk,D,causal,window,dkind", _grid())
def test_fp8_parity_with_the_oracle(B, Sq, Sk, H, Hk, D, causal, window, dkind):
    g = torch.Generator().manual_seed(zlib.crc32(repr((B, Sq, Sk, H, Hk, D, causal, window, dkind)).encode()))
    q, k, v = _fp8((B, Sq, H, D), g, 2.0), _fp8((B, Sk, Hk, D), g, 2.0), _fp8((B, Sk, Hk, D), g)
    ds = _descales(dkind, B, Hk, g)
    scale = D ** -0.5
    out, lse = _run(q, k, v, ds, scale, causal, window)
    assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
    assert _be().last_schedule()["fwd_kernel"] == 4
    _check_parity(q, k, v, ds, scale, causal, window, out, lse)


# ---- varlen, determinism, edge cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,causal,window", [(128, True, (-1, -1)), (64, False, (-1, -1)), (128, False, (48, 8))])
def test_fp8_varlen_matches_per_sequence_calls_bitwise(D, causal, window):
    be = _be()
    g = torch.Generator().manual_seed(7 + D)
    lq, lk = [100, 0, 257, 64, 5, 700], [130, 0, 300, 64, 0, 650]
    B, H, Hk = len(lq), 4, 2
    q, k, v = _fp8((sum(lq), H, D), g, 2.0), _fp8((sum(lk), Hk, D), g, 2.0), _fp8((sum(lk), Hk, D), g)
    qd, kd, vd = _descales("rand", B, Hk, g)
    cq = torch.tensor([0] + list(itertools.accumulate(lq)), dtype=torch.int32, device=DEV)
    ck = torch.tensor([0] + list(itertools.accumulate(lk)), dtype=torch.int32, device=DEV)
    out, lse = be.varlen_fwd_fp8(q.to(DEV), k.to(DEV), v.to(DEV), None, cq, ck, max(lq), max(lk), qd, kd, vd, D ** -0.5, causal,
                                 window[0], window[1])
    assert be.last_schedule()["fwd_kernel"] == 4
    for b in range(B):
        q0, k0 = int(cq[b]), int(ck[b])
        if lq[b] == 0:
            continue
        o1, l1 = be.fwd_fp8(q[q0:q0 + lq[b]][None].to(DEV), k[k0:k0 + lk[b]][None].to(DEV), v[k0:k0 + lk[b]][None].to(DEV), None,
                            qd[b:b + 1], kd[b:b + 1], vd[b:b + 1], D ** -0.5, causal, window[0], window[1])
        assert torch.equal(out[q0:q0 + lq[b]], o1[0]), b
        assert torch.equal(lse[:, q0:q0 + lq[b]], l1[0]), b
        if lk[b] == 0:
            assert (out[q0:q0 + lq[b]] == 0).all() and torch.isinf(lse[:, q0:q0 + lq[b]]).all()


def test_fp8_is_deterministic():
    g = torch.Generator().manual_seed(3)
    q, k, v = _fp8((2, 777, 8, 128), g), _fp8((2, 900, 2, 128), g), _fp8((2, 900, 2, 128), g)
    ds = _descales("rand", 2, 2, g)
    runs = [_run(q, k, v, ds, 0.088, True, (-1, -1)) for _ in range(5)]
    for o, l in runs[1:]:
        assert torch.equal(o, runs[0][0]) and torch.equal(l, runs[0][1])


def test_fp8_empty_keys_and_rows_without_keys():
    g = torch.Generator().manual_seed(4)
    q, k = _fp8((2, 50, 4, 64), g), _fp8((2, 0, 2, 64), g)
    out, lse = _run(q, k, k, (None, None, None), 0.125, False, (-1, -1))
    assert (out == 0).all() and torch.isinf(lse).all() and (lse > 0).all()
    # causal with Sq > Sk: the first Sq - Sk rows see no key
    q, k, v = _fp8((1, 100, 4, 128), g), _fp8((1, 40, 4, 128), g), _fp8((1, 40, 4, 128), g)
    out, lse = _run(q, k, v, (None, None, None), 0.088, True, (-1, -1))
    assert (out[:, :60] == 0).all() and (lse[:, :, :60] == float("inf")).all()
    _check_parity(q, k, v, (None, None, None), 0.088, True, (-1, -1), out, lse)


def test_fp8_out_is_written_in_place():
    g = torch.Generator().manual_seed(5)
    q, k, v = _fp8((2, 130, 4, 128), g), _fp8((2, 130, 4, 128), g), _fp8((2, 130, 4, 128), g)
    ref, _ = _run(q, k, v, (None, None, None), 0.088, False, (-1, -1))
    buf = torch.full((2, 130, 4, 128), float("nan"), dtype=torch.bfloat16, device=DEV)
    out, _ = _run(q, k, v, (None, None, None), 0.088, False, (-1, -1), out_=buf)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf, ref)
    with pytest.raises(RuntimeError, match="bf16"):
        _run(q, k, v, (None, None, None), 0.088, False, (-1, -1), out_=torch.empty(2, 130, 4, 128, dtype=torch.float16, device=DEV))


def test_fp8_extreme_inputs_stay_finite():
    g = torch.Generator().manual_seed(6)
    shape = (1, 300, 4, 128)
    q, k, v = ((torch.sign(torch.randn(shape, generator=g)) * 448.0).to(FP8) for _ in range(3))
    small = tuple(torch.full((1, 4), 1e-3, device=DEV) for _ in range(3))
    for ds in (small, (None, None, None)):
        out, lse = _run(q, k, v, ds, 0.088, True, (-1, -1))
        assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    _check_parity(q, k, v, small, 0.088, True, (-1, -1), *_run(q, k, v, small, 0.088, True, (-1, -1)))


# ---- binders and the public API --------------------------------------------------------------------------------------------------------
def test_fp8_torch_extension_and_ctypes_binder_agree():
    ext = pytest.importorskip("flash_attn_2_cuda")
    be = _be()
    g = torch.Generator().manual_seed(8)
    q, k, v = (_fp8(s, g).to(DEV) for s in ((2, 333, 6, 128), (2, 333, 2, 128), (2, 333, 2, 128)))
    qd, kd, vd = _descales("t", 2, 2, g)
    a = ext.fwd_fp8(q, k, v, None, qd, kd, vd, 0.088, True, -1, -1)
    b = be.fwd_fp8(q, k, v, None, qd, kd, vd, 0.088, True, -1, -1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    cu = torch.tensor([0, 100, 333], dtype=torch.int32, device=DEV)
    qv, kv, vv = q[0], k[0], v[0]
    a = ext.varlen_fwd_fp8(qv, kv, vv, None, cu, cu, 233, 233, qd, kd, vd, 0.088, False, 64, 0)
    b = be.varlen_fwd_fp8(qv, kv, vv, None, cu, cu, 233, 233, qd, kd, vd, 0.088, False, 64, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_fp8_public_api_and_torch_compile():
    from flash_attn_amd import flash_attn_func, flash_attn_varlen_func
    be = _be()
    g = torch.Generator().manual_seed(9)
    q, k, v = (_fp8(s, g).to(DEV) for s in ((2, 200, 8, 64), (2, 260, 2, 64), (2, 260, 2, 64)))
    qd, kd, vd = _descales("rand", 2, 2, g)
    o_be, l_be = be.fwd_fp8(q, k, v, None, qd, kd, vd, 0.1, True, -1, -1)
    out, lse, p = flash_attn_func(q, k, v, softmax_scale=0.1, causal=True, return_attn_probs=True, q_descale=qd, k_descale=kd, v_descale=vd)
    assert p is None and torch.equal(out, o_be) and torch.equal(lse, l_be)
    fn = torch.compile(lambda *a: flash_attn_func(*a[:3], softmax_scale=0.1, causal=True, q_descale=a[3], k_descale=a[4], v_descale=a[5]),
                       fullgraph=True)
    assert torch.equal(fn(q, k, v, qd, kd, vd), o_be)
    cu = torch.tensor([0, 200], dtype=torch.int32, device=DEV)
    cuk = torch.tensor([0, 260], dtype=torch.int32, device=DEV)
    ov = flash_attn_varlen_func(q[0], k[0], v[0], cu, cuk, 200, 260, softmax_scale=0.1, causal=True, q_descale=qd[:1], k_descale=kd[:1],
                                v_descale=vd[:1])
    assert torch.equal(ov, o_be[0])
    with pytest.raises(RuntimeError, match="no backward"):
        flash_attn_func(q.clone().requires_grad_(), k, v)


# ---- the real shapes --------------------------------------------------------------------------------------------------------------------
def test_fp8_config3_shape_against_the_oracle_on_one_unit():
    g = torch.Generator().manual_seed(10)
    B, S, H, D = 4, 4096, 32, 128
    q, k, v = _fp8((B, S, H, D), g), _fp8((B, S, H, D), g), _fp8((B, S, H, D), g)
    ds = _descales("rand", B, H, g)
    out, lse = _run(q, k, v, ds, D ** -0.5, True, (-1, -1))
    assert _be().last_schedule()["name"] == "fa::fa_fwd_fp8_kernel<e4m3,128,4>"
    _check_parity(q, k, v, ds, D ** -0.5, True, (-1, -1), out, lse, rows=(2, 17))


def test_fp8_config5_shape_runs():
    g = torch.Generator().manual_seed(11)
    B, S, H, Hk, D = 2, 8192, 32, 8, 128
    q, k, v = _fp8((B, S, H, D), g), _fp8((B, S, Hk, D), g), _fp8((B, S, Hk, D), g)
    ds = _descales("rand", B, Hk, g)
    out, lse = _run(q, k, v, ds, D ** -0.5, True, (1024, 0))
    assert _be().last_schedule()["fwd_kernel"] == 4
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    _check_parity(q[:, -1500:], k, v, ds, D ** -0.5, True, (1024, 0), out[:, -1500:], lse[:, :, -1500:], rows=(1, 9))
