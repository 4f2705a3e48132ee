"""GPU suite of the FP8 (e4m3) KV cache (csrc/fa_fwd_fp8_kv.hip through fa_kvcache_append + fa_fwd_kvcache_fp8).

Inputs are built on the CPU and copied over; every reference is evaluated on the CPU, over the first cache_seqlens[b] (+ S_new) dequantised rows
of each entry only.
  - one-hot: integer rows that make P exactly one-hot -- an error in page resolution, split ranges or row packing picks the wrong row;
  - parity: the rule of tests/test_fwd_fp8_gpu.py (_check_parity): |out - ref| <= 2 max|emu - ref| + 2 bf16-eps |ref| + 1e-6, ref = the fp64
    oracle on dequantised inputs, emu = fp32 attention with the probabilities rounded to e4m3; the LSE within 5e-4 max(1, |LSE|) of it;
  - poison, addressing bit for bit, the append, the schedule, binders, the public API and the two real decode shapes."""
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
NAN8 = 0x7F   # e4m3 NaN


def _be():
    from flash_attn_amd import backend
    return backend


def _fp8(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(FP8)   # test-input quantisation, on the CPU


def _descales(kind, B, Hk, g):
    """None, contiguous random (0.05, 1.95) or a non-contiguous (Hk, B)^T view, built on the device."""
    if kind is None:
        return None, None, None
    out = []
    for _ in range(3):
        if kind == "rand":
            out.append((torch.rand(B, Hk, generator=g) * 1.9 + 0.05).to(DEV))
        else:
            out.append((torch.rand(Hk, B, generator=g) * 1.9 + 0.05).to(DEV).t())
    return tuple(out)


def _dequant(x, ds, Hk):
    xf = x.to(torch.float64)
    if ds is None:
        return xf.numpy()
    g = x.shape[2] // Hk
    d = ds.detach().cpu().to(torch.float64).repeat_interleave(g, dim=1)   # (B, heads)
    return (xf * d[:, None, :, None]).numpy()


def _emulate(q, k, v, scale, causal, window):
    """fp32 attention on dequantised inputs with the softmax probabilities rounded to e4m3 before the product with V."""
    q, k, v = (torch.from_numpy(x).float() for x in (q, k, v))
    Sq, H, Sk, Hk = q.shape[1], q.shape[2], k.shape[1], k.shape[2]
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
    return torch.einsum("bhts,bshd->bthd", p8, v).double().numpy()


def _check_entry(q, k, v, ds, scale, causal, window, out, lse, head=None):
    """The parity rule on one batch entry: q (1, Sq, H, D), k / v (1, L, Hk, D) = the rows the entry may see, ds = (1, Hk) descales or None;
    out (1, Sq, H, D), lse (1, H, Sq).  head = a query head to restrict the check to.  Prints and returns (max |out - ref|, LSE error)."""
    qd, kd, vd = ds
    if head is not None:
        hk = head // (q.shape[2] // k.shape[2])
        q, k, v = q[:, :, head:head + 1], k[:, :, hk:hk + 1], v[:, :, hk:hk + 1]
        qd, kd, vd = (None if t is None else t[:, hk:hk + 1] for t in (qd, kd, vd))
        out, lse = out[:, :, head:head + 1], lse[:, head:head + 1]
    o = out.detach().cpu().double().numpy()
    l = lse.detach().cpu().double().numpy()
    if k.shape[1] == 0:   # no key at all: out = 0, lse = +inf
        assert (o == 0).all() and (l == np.inf).all()
        return 0.0, 0.0
    Hk = k.shape[2]
    qf, kf, vf = _dequant(q, qd, Hk), _dequant(k, kd, Hk), _dequant(v, vd, Hk)
    ref_o, ref_l = orc.attention_fwd(qf, kf, vf, scale, causal, window)
    emu = _emulate(qf, kf, vf, scale, causal, window)
    assert np.isfinite(o).all()
    tol = 2 * np.abs(emu - ref_o).max() + 2 * BF16_EPS * np.abs(ref_o) + 1e-6
    err_o = np.abs(o - ref_o)
    fin = np.isfinite(ref_l)
    err_l = float((np.abs(l[fin] - ref_l[fin]) / np.maximum(1.0, np.abs(ref_l[fin]))).max()) if fin.any() else 0.0
    print(f"  parity: max|out-ref|={float(err_o.max()):.3e} max|emu-ref|={float(np.abs(emu - ref_o).max()):.3e} lse_err={err_l:.3e}")
    assert (err_o <= tol).all(), (float(err_o.max()), float(np.abs(emu - ref_o).max()))
    assert (np.isfinite(l) == fin).all() and (l[~fin] == np.inf).all()
    assert err_l < 5e-4, err_l
    return float(err_o.max()), err_l


# ---- caches: one logical (B, Sk, Hk, D) content in three addressings --------------------------------------------------------------------
def _bytes(x):
    return x.view(torch.uint8)


def _filled(shape, fill, g):
    """An fp8 tensor of `shape` holding random values (fill = None), zeros or e4m3 NaNs."""
    if fill is None:
        return _fp8(shape, g)
    return torch.full(shape, fill, dtype=torch.uint8).view(FP8)


def _layout(kind, kL, vL, lens_total, g, fill=None):
    """Place the rows [0, lens_total[b]) of the logical caches kL / vL (B, Sk, Hk, D) into a cache of the given kind; everything else -- rows
    past an entry's length, unreferenced cache rows and pages -- holds `fill` (None = random values).  -> (kc, vc, cache_batch_idx, block_table)."""
    B, Sk, Hk, D = kL.shape
    if kind == "contig" or kind == "idx":
        Bc = B if kind == "contig" else B + 2
        rows = list(range(B)) if kind == "contig" else torch.randperm(Bc, generator=g)[:B].tolist()   # a permutation with a gap
        kc, vc = _filled((Bc, Sk, Hk, D), fill, g), _filled((Bc, Sk, Hk, D), fill, g)
        for b in range(B):
            kc[rows[b], :lens_total[b]] = kL[b, :lens_total[b]]
            vc[rows[b], :lens_total[b]] = vL[b, :lens_total[b]]
        idx = None if kind == "contig" else torch.tensor(rows, dtype=torch.int32)
        return kc, vc, idx, None
    page = int(kind[5:])   # "paged256" / "paged512"
    per = Sk // page
    nb = B * per + 3
    order = torch.randperm(nb, generator=g)[:B * per].reshape(B, per)   # pages in shuffled order, three never referenced
    kc, vc = _filled((nb, page, Hk, D), fill, g), _filled((nb, page, Hk, D), fill, g)
    for b in range(B):
        for j in range(per):
            n = max(0, min(page, lens_total[b] - j * page))
            kc[order[b, j], :n] = kL[b, j * page:j * page + n]
            vc[order[b, j], :n] = vL[b, j * page:j * page + n]
    return kc, vc, None, order.to(torch.int32)


def _call(mod, q, kc, vc, kn, vn, lens, idx, bt, ds, scale, causal, window, splits, out_=None):
    dv = lambda t: None if t is None else t.to(DEV)
    return mod.fwd_kvcache_fp8(dv(q), kc, vc, dv(kn), dv(vn), dv(lens), dv(idx), dv(bt), out_, ds[0], ds[1], ds[2], scale, causal,
                               window[0], window[1], splits)


# ---- exact one-hot probe -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("kind", ["contig", "paged256"])
@pytest.mark.parametrize("Sq", [1, 5])
@pytest.mark.parametrize("D", [64, 128])
def test_one_hot_rows_are_exact(D, Sq, kind, splits):
    g = torch.Generator().manual_seed(zlib.crc32(repr((D, Sq, kind, splits)).encode()))
    B, H, Hk, Sk = 3, 8, 2, 1024
    pairs = list(itertools.combinations(range(D), 2))
    sel = torch.randperm(len(pairs), generator=g)[:Sk]
    kL = torch.zeros(B, Sk, Hk, D)
    for j, idx in enumerate(sel.tolist()):
        a, b = pairs[idx]
        kL[:, j, :, a] = 16.0
        kL[:, j, :, b] = 16.0
    lens = [1024, 333, 700]
    tgt = torch.stack([torch.randint(0, lens[b], (Sq, H), generator=g) for b in range(B)])   # (B, Sq, H), inside the entry's length
    q = torch.zeros(B, Sq, H, D)
    for b in range(B):
        for h in range(H):
            q[b, :, h] = kL[b, tgt[b, :, h], h // (H // Hk)]
    # v without zeros: a rescale factor times an earlier row must not show up as a nonzero output element
    vL = (torch.sign(torch.randn(B, Sk, Hk, D, generator=g)) * (0.5 + 3.5 * torch.rand(B, Sk, Hk, D, generator=g))).to(FP8)
    kL = kL.to(FP8)
    qd, kd, vd = ((torch.rand(B, Hk, generator=g) * 1.5 + 0.5) for _ in range(3))
    kc, vc, idx, bt = _layout(kind, kL, vL, lens, g)
    out, lse = _call(_be(), q.to(FP8), kc.to(DEV), vc.to(DEV), None, None, torch.tensor(lens, dtype=torch.int32), idx, bt,
                     (qd.to(DEV), kd.to(DEV), vd.to(DEV)), 1.0, False, (-1, -1), splits)
    sched = _be().last_schedule()
    assert sched["fwd_kernel"] == 5 and sched["fwd_pack"] == 4
    assert (sched["fwd_splits"] == 1) if splits == 1 else (sched["fwd_splits"] > 1)
    rtol = 2e-6 if sched["fwd_splits"] == 1 else 1e-5   # the fp32 merge adds a few roundings
    out, lse = out.cpu(), lse.cpu()
    for b in range(B):
        for h in range(H):
            hk = h // (H // Hk)
            want = (vd[b, hk] * vL[b, tgt[b, :, h], hk].float()).to(torch.bfloat16)
            assert torch.equal(out[b, :, h], want), (b, h, (out[b, :, h].float() - want.float()).abs().max())
            want_l = torch.full((Sq,), 512.0) * qd[b, hk] * kd[b, hk]
            torch.testing.assert_close(lse[b, h], want_l, rtol=rtol, atol=0)


# ---- parity grid ---------------------------------------------------------------------------------------------------------------------------
_SQS = [1, 5, 33, 77, 300]
_HEADS = [(8, 8), (8, 2), (12, 4), (8, 1)]
_MASKS = [(True, (-1, -1)), (False, (-1, -1)), (False, (64, 0))]
_KINDS = ["contig", "idx", "paged256", "paged512"]
_SPLITS = [0, 1, 2, 7, 64]
_DKINDS = [None, "rand", "t"]


def _grid():
    """Every Sq x heads x D x mask; append, addressing, num_splits and the descale kind rotate over the cases (periods 2, 4, 5, 3)."""
    out = []
    for sq, (h, hk), d, (causal, win) in itertools.product(_SQS, _HEADS, (64, 128), _MASKS):
        i = len(out)
        append, kind, splits, dkind = bool((i + i // 6) % 2), _KINDS[(i + i // 5) % 4], _SPLITS[i % 5], _DKINDS[(i + i // 7) % 3]
        out.append(pytest.param(sq, h, hk, d, causal, win, append, kind, splits, dkind,
                                id=f"sq{sq}-h{h}/{hk}-d{d}-{'causal' if causal else 'win%d_%d' % win}-{'append-' if append else ''}{kind}-s{splits}-{dkind}"))
    return out


@pytest.mark.parametrize("Sq,H,Hk,D,causal,window,append,kind,splits,dkind", _grid())
def test_parity_with_the_oracle(Sq, H, Hk, D, causal, window, append, kind, splits, dkind):
    g = torch.Generator().manual_seed(zlib.crc32(repr((Sq, H, Hk, D, causal, window, append, kind, splits, dkind)).encode()))
    B, Sk = 4, 1024
    s_new = Sq if append else 0
    full = Sk - s_new
    lens = [0, full, int(torch.randint(1, full, (1,), generator=g)), int(torch.randint(1, 130, (1,), generator=g))]   # uneven, with 0 and Sk
    q = _fp8((B, Sq, H, D), g, 2.0)
    kL, vL = _fp8((B, Sk, Hk, D), g, 2.0), _fp8((B, Sk, Hk, D), g)
    kn = vn = None
    if append:   # the new rows are the logical rows lens[b] .. lens[b] + S_new; the cache holds something else there before the call
        kn = torch.stack([kL[b, lens[b]:lens[b] + s_new] for b in range(B)])
        vn = torch.stack([vL[b, lens[b]:lens[b] + s_new] for b in range(B)])
    kc, vc, idx, bt = _layout(kind, kL, vL, lens, g)
    ds = _descales(dkind, B, Hk, g)
    scale = D ** -0.5
    out, lse = _call(_be(), q, kc.to(DEV), vc.to(DEV), kn, vn, torch.tensor(lens, dtype=torch.int32), idx, bt, ds, scale, causal, window, splits)
    assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32 and out.shape == (B, Sq, H, D) and lse.shape == (B, H, Sq)
    sched = _be().last_schedule()
    assert sched["fwd_kernel"] == 5
    assert sched["fwd_pack"] == (H // Hk if (H // Hk) * Sq <= 128 else 1)
    if splits == 1 or Sq > 128:
        assert sched["fwd_splits"] == 1
    elif splits > 1:
        assert sched["fwd_splits"] > 1
    for b in range(B):
        L = lens[b] + s_new
        dsb = tuple(None if t is None else t[b:b + 1] for t in ds)
        _check_entry(q[b:b + 1], kL[b:b + 1, :L], vL[b:b + 1, :L], dsb, scale, causal, window, out[b:b + 1], lse[b:b + 1])


# ---- poison: nothing behind an entry's length, and no unreferenced page, is ever read ------------------------------------------------------------
@pytest.mark.parametrize("kind", _KINDS)
@pytest.mark.parametrize("Sq,splits", [(1, 0), (1, 1), (5, 3), (77, 1), (300, 0)])
def test_bytes_past_the_length_are_never_read(kind, Sq, splits):
    g = torch.Generator().manual_seed(zlib.crc32(repr((kind, Sq, splits)).encode()))
    B, Sk, H, Hk, D = 3, 1024, 8, 2, 128
    lens = [Sk - 1, 1, 517]
    q, kL, vL = _fp8((B, Sq, H, D), g), _fp8((B, Sk, Hk, D), g), _fp8((B, Sk, Hk, D), g)
    ds = _descales("rand", B, Hk, g)
    res = []
    for fill in (0, NAN8):
        gl = torch.Generator().manual_seed(5)   # the same placement both times
        kc, vc, idx, bt = _layout(kind, kL, vL, lens, gl, fill=fill)
        res.append(_call(_be(), q, kc.to(DEV), vc.to(DEV), None, None, torch.tensor(lens, dtype=torch.int32), idx, bt, ds, D ** -0.5, True,
                         (-1, -1), splits))
    (o0, l0), (o1, l1) = res
    assert torch.isfinite(o1.float()).all()
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


# ---- the same kernel under different addressing: bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq,H,Hk,D,splits", [(1, 8, 2, 128, 1), (1, 8, 2, 128, 3), (5, 12, 4, 64, 0), (77, 8, 8, 128, 2), (300, 8, 1, 64, 1)])
def test_addressing_does_not_change_a_bit(Sq, H, Hk, D, splits):
    g = torch.Generator().manual_seed(zlib.crc32(repr((Sq, H, Hk, D, splits)).encode()))
    B, Sk = 3, 1024
    lens = [1000, 64, 511]
    q, kL, vL = _fp8((B, Sq, H, D), g), _fp8((B, Sk, Hk, D), g), _fp8((B, Sk, Hk, D), g)
    ds = _descales("t", B, Hk, g)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    runs = {}
    for kind in _KINDS:
        kc, vc, idx, bt = _layout(kind, kL, vL, lens, g)
        runs[kind] = _call(_be(), q, kc.to(DEV), vc.to(DEV), None, None, lens_t, idx, bt, ds, D ** -0.5, True, (-1, -1), splits)
    for kind in _KINDS[1:]:   # paged vs contiguous, cache_batch_idx vs the pre-gathered (contiguous) cache
        assert torch.equal(runs[kind][0], runs["contig"][0]) and torch.equal(runs[kind][1], runs["contig"][1]), kind
    kc, vc, idx, bt = _layout("paged256", kL, vL, lens, g)
    kc, vc = kc.to(DEV), vc.to(DEV)
    for _ in range(5):
        o, l = _call(_be(), q, kc, vc, None, None, lens_t, idx, bt, ds, D ** -0.5, True, (-1, -1), splits)
        assert torch.equal(o, runs["contig"][0]) and torch.equal(l, runs["contig"][1])


# ---- the append is a byte copy into the right rows and touches nothing else ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", _KINDS)
@pytest.mark.parametrize("s_new,D", [(1, 128), (5, 64), (300, 128)])
def test_append_writes_the_new_rows_and_nothing_else(kind, s_new, D):
    g = torch.Generator().manual_seed(zlib.crc32(repr((kind, s_new, D)).encode()))
    B, Sk, H, Hk = 3, 1024, 4, 2
    lens = [0, Sk - s_new, 255]
    q, kL, vL = _fp8((B, s_new, H, D), g), _fp8((B, Sk, Hk, D), g), _fp8((B, Sk, Hk, D), g)
    kc, vc, idx, bt = _layout(kind, kL, vL, lens, g)
    # new rows of every byte value but the NaNs' (a NaN in a visible row would reach the output; the copy is checked on bytes)
    kn = torch.randint(0, 127, (B, s_new, Hk, D), generator=g, dtype=torch.uint8).view(FP8)
    vn = (torch.randint(0, 127, (B, s_new, Hk, D), generator=g, dtype=torch.uint8) + 128).view(FP8)
    kd_, vd_ = kc.to(DEV), vc.to(DEV)
    out, _ = _call(_be(), q, kd_, vd_, kn, vn, torch.tensor(lens, dtype=torch.int32), idx, bt, (None, None, None), D ** -0.5, True, (-1, -1), 0)
    assert torch.isfinite(out.float()).all()
    want_k, want_v = _bytes(kc).clone(), _bytes(vc).clone()
    for b in range(B):
        for t in range(s_new):
            row = lens[b] + t
            if bt is not None:
                page = kc.shape[1]
                want_k[bt[b, row // page], row % page] = _bytes(kn)[b, t]
                want_v[bt[b, row // page], row % page] = _bytes(vn)[b, t]
            else:
                r = b if idx is None else int(idx[b])
                want_k[r, row] = _bytes(kn)[b, t]
                want_v[r, row] = _bytes(vn)[b, t]
    assert torch.equal(_bytes(kd_.cpu()), want_k) and torch.equal(_bytes(vd_.cpu()), want_v)


# ---- schedule ---------------------------------------------------------------------------------------------------------------------------------
def test_schedule_kernel_id_packing_and_splits():
    be = _be()
    g = torch.Generator().manual_seed(21)
    for Sq, H, Hk, D, pack in [(1, 8, 2, 128, 4), (5, 12, 4, 64, 3), (32, 8, 2, 128, 4), (33, 8, 2, 128, 1), (16, 8, 1, 64, 8), (17, 8, 1, 64, 1), (4, 8, 8, 128, 1)]:
        q, kc = _fp8((2, Sq, H, D), g), _fp8((2, 512, Hk, D), g).to(DEV)
        _call(be, q, kc, kc, None, None, None, None, None, (None, None, None), 0.1, True, (-1, -1), 0)
        s = be.last_schedule()
        assert s["fwd_kernel"] == 5 and s["fwd_pack"] == pack and s["d"] == D and s["fwd_nw"] == 4, (Sq, H, Hk, s)
        assert s["name"].startswith(f"fa::fa_fwd_fp8_kv_kernel<e4m3,{D},")
    assert be.FWD_KERNEL_NAMES[5] == "fa_fwd_fp8_kv_kernel"
    q, kc = _fp8((1, 1, 8, 128), g), _fp8((1, 8192, 2, 128), g).to(DEV)
    _call(be, q, kc, kc, None, None, None, None, None, (None, None, None), 0.1, False, (-1, -1), 0)
    assert be.last_schedule()["fwd_splits"] > 1
    _call(be, q, kc, kc, None, None, None, None, None, (None, None, None), 0.1, False, (-1, -1), 1)
    assert be.last_schedule()["fwd_splits"] == 1
    # the bf16 cache path is untouched by the new kernel id
    qb, kb = torch.randn(1, 1, 8, 128, dtype=torch.bfloat16, device=DEV), torch.randn(1, 512, 2, 128, dtype=torch.bfloat16, device=DEV)
    be.fwd_kvcache(qb, kb, kb, None, None, None, None, None, None, None, None, None, None, 0.1, False, -1, -1, 0.0, True, 0)
    assert be.last_schedule()["fwd_kernel"] == 1


# ---- binders and the public API ---------------------------------------------------------------------------------------------------------------
def test_torch_extension_and_ctypes_binder_agree():
    ext = pytest.importorskip("flash_attn_2_cuda")
    be = _be()
    g = torch.Generator().manual_seed(8)
    B, Sk, H, Hk, D = 3, 1024, 8, 2, 128
    lens = [5, 900, 300]
    kL, vL = _fp8((B, Sk, Hk, D), g), _fp8((B, Sk, Hk, D), g)
    ds = _descales("t", B, Hk, g)
    for kind, Sq, splits, causal, window in [("contig", 1, 0, False, (-1, -1)), ("idx", 5, 3, True, (-1, -1)), ("paged256", 77, 1, False, (64, 0)),
                                             ("paged512", 300, 0, True, (-1, -1))]:
        q, kn, vn = _fp8((B, Sq, H, D), g), _fp8((B, min(Sq, 100), Hk, D), g), _fp8((B, min(Sq, 100), Hk, D), g)
        kc, vc, idx, bt = _layout(kind, kL, vL, lens, g)
        res = []
        for mod in (ext, be):
            kd_, vd_ = kc.to(DEV), vc.to(DEV)
            o, l = _call(mod, q, kd_, vd_, kn, vn, torch.tensor(lens, dtype=torch.int32), idx, bt, ds, 0.088, causal, window, splits)
            res.append((o, l, kd_, vd_))
        for x, y in zip(*res):
            assert torch.equal(_bytes(x) if x.dtype == FP8 else x, _bytes(y) if y.dtype == FP8 else y), kind
    for mod in (ext, be):   # the guards the bf16 binder carries
        q, kc = _fp8((2, 1, 4, 64), g).to(DEV), _fp8((4, 256, 2, 64), g).to(DEV)
        bt = torch.tensor([[0, 1], [2, 3]], dtype=torch.int32, device=DEV)
        one = torch.ones(2, dtype=torch.int32, device=DEV)
        with pytest.raises(RuntimeError, match="does not support cache_batch_idx"):
            mod.fwd_kvcache_fp8(q, kc, kc, None, None, None, one, bt, None, None, None, None, 0.1, False, -1, -1, 0)
        with pytest.raises(RuntimeError, match="exceeds the capacity"):
            mod.fwd_kvcache_fp8(q, kc, kc, None, None, one * 513, None, bt, None, None, None, None, 0.1, False, -1, -1, 0)
        big = _fp8((2, 300, 2, 64), g).to(DEV)
        with pytest.raises(RuntimeError, match="seqlen <= the seqlen of the KV cache"):
            mod.fwd_kvcache_fp8(q, kc[:2], kc[:2], big, big, one, None, None, None, None, None, None, 0.1, False, -1, -1, 0)
        with pytest.raises(RuntimeError, match="mixed dtypes"):
            mod.fwd_kvcache_fp8(q.to(torch.bfloat16), kc[:2], kc[:2], None, None, None, None, None, None, None, None, None, 0.1, False, -1, -1, 0)
        q96 = _fp8((2, 1, 4, 96), g).to(DEV)
        kc96 = _fp8((2, 256, 2, 96), g).to(DEV)
        with pytest.raises(RuntimeError, match="head dim 96"):
            mod.fwd_kvcache_fp8(q96, kc96, kc96, None, None, None, None, None, None, None, None, None, 0.1, False, -1, -1, 0)


def test_public_api_matches_the_binder():
    from flash_attn_amd import flash_attn_with_kvcache
    be = _be()
    g = torch.Generator().manual_seed(9)
    B, Sk, H, Hk, D = 2, 768, 8, 2, 64
    q, kn, vn = (_fp8(s, g).to(DEV) for s in ((B, 3, H, D), (B, 3, Hk, D), (B, 3, Hk, D)))
    kc, vc = _fp8((B, Sk, Hk, D), g), _fp8((B, Sk, Hk, D), g)
    qd, kd, vd = _descales("rand", B, Hk, g)
    lens = torch.full((B,), 400, dtype=torch.int32, device=DEV)
    k1, v1 = kc.to(DEV), vc.to(DEV)
    o_be, l_be = be.fwd_kvcache_fp8(q, k1, v1, kn, vn, lens, None, None, None, qd, kd, vd, 0.1, True, -1, -1, 0)
    k2, v2 = kc.to(DEV), vc.to(DEV)
    out, lse = flash_attn_with_kvcache(q, k2, v2, k=kn, v=vn, cache_seqlens=400, softmax_scale=0.1, causal=True, return_softmax_lse=True,
                                       q_descale=qd, k_descale=kd, v_descale=vd)   # an int cache_seqlens
    assert out.dtype == torch.bfloat16 and torch.equal(out, o_be) and torch.equal(lse, l_be)
    assert torch.equal(_bytes(k1), _bytes(k2)) and torch.equal(_bytes(v1), _bytes(v2)) and not torch.equal(_bytes(k2.cpu()), _bytes(kc))
    out2 = flash_attn_with_kvcache(q, k2, v2, cache_seqlens=lens + 3, softmax_scale=0.1, causal=True, q_descale=qd, k_descale=kd, v_descale=vd)
    assert torch.equal(out2, o_be)   # the rows are in the cache now
    # default scale, a paged cache, forced splits
    bt = torch.tensor([[2, 0, 1], [5, 3, 4]], dtype=torch.int32, device=DEV)
    kp = k2.reshape(B * 3, 256, Hk, D)[torch.tensor([1, 2, 0, 4, 5, 3], device=DEV)].contiguous()
    vp = v2.reshape(B * 3, 256, Hk, D)[torch.tensor([1, 2, 0, 4, 5, 3], device=DEV)].contiguous()
    a = flash_attn_with_kvcache(q, k2, v2, cache_seqlens=lens + 3, causal=True, num_splits=2, k_descale=kd)
    b = flash_attn_with_kvcache(q, kp, vp, cache_seqlens=lens + 3, causal=True, num_splits=2, k_descale=kd, block_table=bt)
    assert torch.equal(a, b) and _be().last_schedule()["fwd_splits"] == 2
    # out_ of the binder is written in place
    buf = torch.full((B, 3, H, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    o3, _ = be.fwd_kvcache_fp8(q, k2, v2, None, None, lens + 3, None, None, buf, qd, kd, vd, 0.1, True, -1, -1, 0)
    assert o3.data_ptr() == buf.data_ptr() and torch.equal(buf, o_be)
    with pytest.raises(RuntimeError, match="bf16|BF16"):
        be.fwd_kvcache_fp8(q, k2, v2, None, None, lens, None, None, torch.empty(B, 3, H, D, dtype=torch.float16, device=DEV), qd, kd, vd, 0.1,
                           True, -1, -1, 0)


def test_prefill_then_decode_against_the_cache_it_filled():
    from flash_attn_amd import flash_attn_func, flash_attn_with_kvcache
    g = torch.Generator().manual_seed(12)
    B, P, steps, H, Hk, D, Sk = 2, 200, 4, 8, 2, 128, 512
    scale = D ** -0.5
    q_all, k_all, v_all = _fp8((B, P + steps, H, D), g, 2.0), _fp8((B, P + steps, Hk, D), g, 2.0), _fp8((B, P + steps, Hk, D), g)
    ds = _descales("rand", B, Hk, g)
    qd, kd, vd = ds
    kc = torch.zeros(B, Sk, Hk, D, dtype=torch.uint8, device=DEV).view(FP8)
    vc = torch.zeros(B, Sk, Hk, D, dtype=torch.uint8, device=DEV).view(FP8)
    # prefill: the fp8 forward on the prompt, and the same prompt through the cache path, which stores its k / v
    o_pre, l_pre, _ = flash_attn_func(q_all[:, :P].to(DEV), k_all[:, :P].to(DEV), v_all[:, :P].to(DEV), causal=True, return_attn_probs=True,
                                      q_descale=qd, k_descale=kd, v_descale=vd)
    o_fill, l_fill = flash_attn_with_kvcache(q_all[:, :P].to(DEV), kc, vc, k=k_all[:, :P].to(DEV), v=v_all[:, :P].to(DEV), cache_seqlens=0,
                                             causal=True, return_softmax_lse=True, q_descale=qd, k_descale=kd, v_descale=vd)
    assert torch.equal(_bytes(kc[:, :P].cpu()), _bytes(k_all[:, :P])) and torch.equal(_bytes(vc[:, :P].cpu()), _bytes(v_all[:, :P]))
    for b in range(B):
        dsb = tuple(t[b:b + 1] for t in ds)
        for o, l in ((o_pre, l_pre), (o_fill, l_fill)):
            _check_entry(q_all[b:b + 1, :P], k_all[b:b + 1, :P], v_all[b:b + 1, :P], dsb, scale, True, (-1, -1), o[b:b + 1], l[b:b + 1])
    for t in range(steps):
        n = P + t
        out, lse = flash_attn_with_kvcache(q_all[:, n:n + 1].to(DEV), kc, vc, k=k_all[:, n:n + 1].to(DEV), v=v_all[:, n:n + 1].to(DEV),
                                           cache_seqlens=n, causal=True, return_softmax_lse=True, q_descale=qd, k_descale=kd, v_descale=vd)
        assert _be().last_schedule()["fwd_kernel"] == 5
        for b in range(B):
            dsb = tuple(x[b:b + 1] for x in ds)
            _check_entry(q_all[b:b + 1, n:n + 1], k_all[b:b + 1, :n + 1], v_all[b:b + 1, :n + 1], dsb, scale, False, (-1, -1), out[b:b + 1],
                         lse[b:b + 1])
    assert torch.equal(_bytes(kc[:, :P + steps].cpu()), _bytes(k_all)) and (_bytes(kc[:, P + steps:]) == 0).all()


# ---- the real decode shapes ---------------------------------------------------------------------------------------------------------------------
def test_decode_b64_sk16k_on_one_sampled_unit():
    g = torch.Generator().manual_seed(13)
    B, Sk, H, Hk, D = 64, 16384, 32, 8, 128
    q = _fp8((B, 1, H, D), g, 2.0)
    kc = torch.randn((B, Sk, Hk, D), generator=g, dtype=torch.bfloat16).to(FP8)
    vc = torch.randn((B, Sk, Hk, D), generator=g, dtype=torch.bfloat16).to(FP8)
    lens = torch.randint(Sk // 2, Sk + 1, (B,), generator=g).to(torch.int32)
    lens[7] = Sk
    ds = _descales("rand", B, Hk, g)
    out, lse = _call(_be(), q, kc.to(DEV), vc.to(DEV), None, None, lens, None, None, ds, D ** -0.5, False, (-1, -1), 0)
    s = _be().last_schedule()
    assert s["fwd_kernel"] == 5 and s["fwd_pack"] == 4
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    for b, h in ((41, 13), (7, 30)):
        L = int(lens[b])
        dsb = tuple(t[b:b + 1] for t in ds)
        _check_entry(q[b:b + 1], kc[b:b + 1, :L], vc[b:b + 1, :L], dsb, D ** -0.5, False, (-1, -1), out[b:b + 1], lse[b:b + 1], head=h)


def test_decode_b1_sk128k_with_the_heuristic_splits():
    g = torch.Generator().manual_seed(14)
    B, Sk, H, Hk, D = 1, 131072, 32, 8, 128
    q, kc, vc = _fp8((B, 1, H, D), g, 2.0), _fp8((B, Sk, Hk, D), g), _fp8((B, Sk, Hk, D), g)
    lens = torch.tensor([Sk - 77], dtype=torch.int32)
    ds = _descales("rand", B, Hk, g)
    out, lse = _call(_be(), q, kc.to(DEV), vc.to(DEV), None, None, lens, None, None, ds, D ** -0.5, False, (-1, -1), 0)
    s = _be().last_schedule()
    assert s["fwd_kernel"] == 5 and s["fwd_splits"] > 1 and s["fwd_pack"] == 4
    L = int(lens[0])
    _check_entry(q, kc[:, :L], vc[:, :L], ds, D ** -0.5, False, (-1, -1), out, lse, head=21)
