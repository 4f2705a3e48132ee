"""GPU suite of the absorbed MLA decode: q / k head dim 576, v / o head dim 512, v_cache = k_cache[..., :512] (csrc/fa_fwd_mla.hip through
fa_kvcache_append + fa_fwd_kvcache).

Inputs are built on the CPU and copied over; references are tests/_util.attention_torch over the first cache_seqlens[b] (+ S_new) rows of each
entry only.  Kernel 7 is asserted after every call.
  - one-hot: rows that make P exactly one-hot (two channels of 16 drawn from all 576; many pairs differ only in channels >= 512): a dropped rotary
    k-step, a V read from the wrong channels, a wrong page, split range or row packing picks another row;
  - parity: the rule of tests/test_headdim_v_gpu.py::_check -- |out - fp32 ref| <= 2 x (error of the same-dtype PyTorch evaluation) + 1e-4, LSE within
    2e-3, +inf exactly where no key is visible;
  - poison (NaN behind every length, in unreferenced rows and pages; guard columns behind out's 512), the append, addressings / binders / repeats
    bit for bit, a non-contiguous row stride."""
import itertools
import zlib

import pytest
import torch

from tests._util import attention_torch, max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, DV = 576, 512
SCALE = D ** -0.5
BF, HF = torch.bfloat16, torch.float16


def _be():
    from flash_attn_amd import backend
    return backend


def _assert_mla(dtype, pack, splits=None):
    s = _be().last_schedule()
    assert s["fwd_kernel"] == 7 and s["d"] == D and s["dv"] == DV and s["fwd_pack"] == pack, s
    assert s["name"].startswith("fa::fa_fwd_mla_kernel<%s,576,512" % ("bf16" if dtype == BF else "f16")), s
    assert _be().FWD_KERNEL_NAMES[7] == "fa_fwd_mla_kernel"
    if splits is not None:
        assert (s["fwd_splits"] == 1) if splits == 1 else (s["fwd_splits"] > 1), s
    return s


def _same(a, b):
    raw = lambda x: x.contiguous().view(torch.int16 if x.dtype in (BF, HF) else torch.int32)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw(a), raw(b))


# ---- caches: one logical (B, Sk, Hk, 576) content in three addressings ------------------------------------------------------------------------
def _filled(shape, fill, g, dtype):
    if fill is None:
        return torch.randn(shape, generator=g).to(dtype)
    return torch.full(shape, fill, dtype=dtype)


def _layout(kind, kL, lens_total, g, fill=None, width=D):
    """Place rows [0, lens_total[b]) of the logical cache kL into a cache of the given kind, allocated `width` channels wide (>= 576: a free row
    stride); everything else -- rows past an entry's length, unreferenced cache rows and pages -- holds `fill` (None = random values).
    -> (kc (.., 576) on the device, cache_batch_idx, block_table)."""
    B, Sk, Hk, _ = kL.shape
    if kind in ("contig", "idx"):
        Bc = B if kind == "contig" else B + 2
        rows = list(range(B)) if kind == "contig" else torch.randperm(Bc, generator=g)[:B].tolist()   # a permutation with a gap
        kc = _filled((Bc, Sk, Hk, width), fill, g, kL.dtype)
        for b in range(B):
            kc[rows[b], :lens_total[b], :, :D] = kL[b, :lens_total[b]]
        idx = None if kind == "contig" else torch.tensor(rows, dtype=torch.int32)
        return kc.to(DEV)[..., :D], idx, None
    page = int(kind[5:])   # "paged256" / "paged512"
    per = Sk // page
    nb = B * per + 3
    order = torch.randperm(nb, generator=g)[:B * per].reshape(B, per)   # pages in shuffled order, three never referenced
    kc = _filled((nb, page, Hk, width), fill, g, kL.dtype)
    for b in range(B):
        for j in range(per):
            n = max(0, min(page, lens_total[b] - j * page))
            kc[order[b, j], :n, :, :D] = kL[b, j * page:j * page + n]
    return kc.to(DEV)[..., :D], None, order.to(torch.int32)


def _call(mod, q, kc, lens, idx, bt, causal=False, window=(-1, -1), splits=0, kn=None, vn=None, out_=None, scale=SCALE):
    dv = lambda t: None if t is None else t.to(DEV)
    return mod.fwd_kvcache(dv(q), kc, kc[..., :DV], kn, vn, dv(lens), None, None, dv(idx), None, dv(bt), None, out_, scale, causal, window[0], window[1],
                           0.0, True, splits)


# ---- exact one-hot probe -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("kind", ["contig", "paged256"])
@pytest.mark.parametrize("Sq", [1, 5])
@pytest.mark.parametrize("H,Hk", [(16, 1), (8, 2)])
def test_one_hot_rows_are_exact(H, Hk, Sq, kind, splits, dtype):
    g = torch.Generator().manual_seed(zlib.crc32(repr((H, Hk, Sq, kind, splits)).encode()))
    B, Sk = 3, 1024
    pairs = list(itertools.combinations(range(D), 2))
    kL = torch.zeros(B, Sk, Hk, D)
    for hk in range(Hk):   # every KV head draws its own pairs: a wrong KV-head index picks another row
        sel = torch.randperm(len(pairs), generator=g)[:Sk]
        for j, idx in enumerate(sel.tolist()):
            a, b = pairs[idx]
            kL[:, j, hk, a] = 16.0
            kL[:, j, hk, b] = 16.0
    lens = [1024, 333, 700]
    tgt = torch.stack([torch.randint(0, lens[b], (Sq, H), generator=g) for b in range(B)])   # (B, Sq, H), inside the entry's length
    q = torch.zeros(B, Sq, H, D)
    for b in range(B):
        for h in range(H):
            q[b, :, h] = kL[b, tgt[b, :, h], h // (H // Hk)]
    kL = kL.to(dtype)
    kc, idx, bt = _layout(kind, kL, lens, g)
    out, lse = _call(_be(), q.to(dtype), kc, torch.tensor(lens, dtype=torch.int32), idx, bt, scale=1.0, splits=splits)
    _assert_mla(dtype, H // Hk, splits)
    out, lse = out.cpu(), lse.cpu()
    assert out.shape == (B, Sq, H, DV) and lse.shape == (B, H, Sq)
    for b in range(B):
        for h in range(H):
            want = kL[b, tgt[b, :, h], h // (H // Hk), :DV]
            assert torch.equal(out[b, :, h], want), (b, h, (out[b, :, h].float() - want.float()).abs().max())
    assert torch.equal(lse, torch.full_like(lse, 512.0)), (lse - 512.0).abs().max()


# ---- parity grid ---------------------------------------------------------------------------------------------------------------------------
_SHAPES = [(128, 1, 1, False, (-1, -1)), (128, 1, 2, True, (-1, -1)), (16, 1, 1, False, (-1, -1)), (8, 2, 3, False, (-1, -1)), (4, 4, 130, True, (200, -1))]
_LENS = [0, 1, 5, 64, 333, 1024]
_SK = 1024
_KINDS = ["contig", "idx", "paged256", "paged512"]
_REF = {}


def _problem(shape, dtype):
    """q, the logical cache and the per-entry references (fp32 and same-dtype PyTorch) of one shape: computed once, shared, never modified."""
    key = (shape, dtype)
    if key not in _REF:
        H, Hk, Sq, causal, window = shape
        g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
        B = len(_LENS)
        q = torch.randn(B, Sq, H, D, generator=g).to(dtype)
        kL = torch.randn(B, _SK, Hk, D, generator=g).to(dtype)
        o32 = torch.zeros(B, Sq, H, DV)
        l32 = torch.full((B, H, Sq), float("inf"))
        base = 0.0
        for b, L in enumerate(_LENS):
            if L == 0:
                continue
            qb, kb = q[b:b + 1].to(DEV), kL[b:b + 1, :L].to(DEV)
            o, l = attention_torch(qb.float(), kb.float(), kb[..., :DV].float(), causal, window, SCALE, True)
            opt, _ = attention_torch(qb, kb, kb[..., :DV], causal, window, SCALE, False)
            o32[b], l32[b] = o[0].cpu(), l[0].cpu()
            base = max(base, max_abs(opt.float(), o))
        _REF[key] = (q, kL, o32, l32, base)
    return _REF[key]


def _check(out, lse, ref, what):
    _, _, o32, l32, base = ref
    e = max_abs(out.float().cpu(), o32)
    fin = torch.isfinite(l32)
    el = max_abs(lse.cpu()[fin], l32[fin])
    print(f"{what} out err {e:.3e} (pytorch {base:.3e}) lse err {el:.3e}")
    assert e <= 2 * base + 1e-4
    assert el < 2e-3 and torch.equal(torch.isposinf(lse.cpu()), ~fin)


@pytest.mark.parametrize("splits", [1, 0, 3, 7])
@pytest.mark.parametrize("kind", _KINDS)
@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "H%d_Hk%d_Sq%d" % s[:3])
def test_parity(shape, kind, splits):
    H, Hk, Sq, causal, window = shape
    ref = _problem(shape, BF)
    q, kL = ref[0], ref[1]
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, kind, splits)).encode()))
    kc, idx, bt = _layout(kind, kL, _LENS, g)
    out, lse = _call(_be(), q, kc, torch.tensor(_LENS, dtype=torch.int32), idx, bt, causal, window, splits)
    s = _assert_mla(BF, H // Hk)
    if splits > 1:   # forced splits are honoured while the packed rows fit 128; (7 splits of 16 tiles: ranges of 3 tiles, the last split of short entries is empty)
        assert (s["fwd_splits"] > 1) == (H // Hk * Sq <= 128), s
    _check(out, lse, ref, f"{shape[:3]} {kind} splits={splits}")


@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "H%d_Hk%d_Sq%d" % s[:3])
def test_parity_fp16(shape):
    H, Hk, Sq, causal, window = shape
    ref = _problem(shape, HF)
    g = torch.Generator().manual_seed(11)
    kc, idx, bt = _layout("paged256", ref[1], _LENS, g)
    out, lse = _call(_be(), ref[0], kc, torch.tensor(_LENS, dtype=torch.int32), idx, bt, causal, window, 0)
    _assert_mla(HF, H // Hk)
    _check(out, lse, ref, f"fp16 {shape[:3]}")


def test_int_cache_seqlens_and_the_public_function():
    from flash_attn_amd import flash_attn_with_kvcache
    shape = _SHAPES[2]
    q, kL, o32, l32, base = _problem(shape, BF)
    kc = kL.to(DEV)
    out, lse = flash_attn_with_kvcache(q.to(DEV), kc, kc[..., :DV], cache_seqlens=333, return_softmax_lse=True)   # default scale = 576 ** -0.5
    _assert_mla(BF, 16)
    b = _LENS.index(333)
    e = max_abs(out[b].float().cpu(), o32[b])
    print(f"public out err {e:.3e} (pytorch {base:.3e})")
    assert out.shape == (len(_LENS), 1, 16, DV) and e <= 2 * base + 1e-4 and max_abs(lse[b].cpu(), l32[b]) < 2e-3


# ---- poison --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("kind", ["contig", "idx", "paged256"])
@pytest.mark.parametrize("shape", [_SHAPES[2], _SHAPES[3]], ids=lambda s: "H%d_Hk%d_Sq%d" % s[:3])
def test_poison_behind_lengths_and_guard_columns(shape, kind, splits):
    H, Hk, Sq, causal, window = shape
    q, kL = _problem(shape, BF)[:2]
    B = len(_LENS)
    res = []
    for fill in (0.0, float("nan")):
        g = torch.Generator().manual_seed(5)   # the same placement for both fills
        kc, idx, bt = _layout(kind, kL, _LENS, g, fill=fill)
        buf = torch.full((B, Sq, H, DV + 64), -7.0, device=DEV, dtype=BF)
        out, lse = _call(_be(), q, kc, torch.tensor(_LENS, dtype=torch.int32), idx, bt, causal, window, splits, out_=buf[..., :DV])
        _assert_mla(BF, H // Hk)
        assert out.data_ptr() == buf.data_ptr()
        assert bool((buf[..., DV:] == -7.0).all()), "guard columns behind out were written"
        res.append((out.cpu(), lse.cpu()))
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1])
    assert bool(torch.isfinite(res[1][0]).all())


# ---- append --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", [False, True], ids=["v_none", "v_view"])
@pytest.mark.parametrize("s_new", [1, 3])
@pytest.mark.parametrize("kind", ["contig", "idx", "paged256"])
def test_append_writes_the_rows_once(kind, s_new, view):
    g = torch.Generator().manual_seed(zlib.crc32(repr((kind, s_new, view)).encode()))
    B, Sk, H, Hk, Sq = 4, 512, 8, 2, 2
    lens = [0, 255, 300, 509]   # 255 + 3 crosses a page; 509 + 3 fills the cache
    kL = torch.randn(B, Sk, Hk, D, generator=g).to(BF)
    kn = torch.randn(B, s_new, Hk, D, generator=g).to(BF)
    q = torch.randn(B, Sq, H, D, generator=g).to(BF)
    kc, idx, bt = _layout(kind, kL, lens, g)
    want = kc.clone()   # CPU-side copy of the append: same addressing arithmetic as _layout
    rows = list(range(B)) if idx is None else idx.tolist()
    for b in range(B):
        for t in range(s_new):
            r = lens[b] + t
            if bt is None:
                want[rows[b], r] = kn[b, t].to(DEV)
            else:
                want[int(bt[b, r // 256]), r % 256] = kn[b, t].to(DEV)
    knd = kn.to(DEV)
    out, lse = _call(_be(), q, kc, torch.tensor(lens, dtype=torch.int32), idx, bt, True, (-1, -1), 0, kn=knd, vn=knd[..., :DV] if view else None)
    _assert_mla(BF, H // Hk)
    assert _same(kc, want), "cache bytes after the append differ from the CPU-side copy (or rows outside the append were touched)"
    out2, lse2 = _call(_be(), q, want, torch.tensor([l + s_new for l in lens], dtype=torch.int32), idx, bt, True, (-1, -1), 0)
    _assert_mla(BF, H // Hk)
    assert _same(out, out2) and _same(lse, lse2)


@pytest.mark.parametrize("view", [False, True], ids=["v_none", "v_view"])
@pytest.mark.parametrize("kind", ["contig", "paged256"])
def test_append_through_the_torch_extension_matches_the_ctypes_binder(kind, view):
    import flash_attn_2_cuda as ext
    g = torch.Generator().manual_seed(zlib.crc32(repr((kind, view)).encode()))
    B, Sk, H, Hk, Sq, s_new = 3, 512, 8, 2, 2, 3
    lens = torch.tensor([0, 255, 509], dtype=torch.int32)
    kL = torch.randn(B, Sk, Hk, D, generator=g).to(BF)
    knd = torch.randn(B, s_new, Hk, D, generator=g).to(BF).to(DEV)
    q = torch.randn(B, Sq, H, D, generator=g).to(BF)
    kc, idx, bt = _layout(kind, kL, lens.tolist(), g)
    res = []
    for mod in (_be(), ext):
        cache = kc.clone()
        out, lse = _call(mod, q, cache, lens, idx, bt, True, (-1, -1), 0, kn=knd, vn=knd[..., :DV] if view else None)
        _assert_mla(BF, H // Hk)
        res.append((cache, out.cpu(), lse.cpu()))
    assert not _same(res[0][0], kc), "the append wrote nothing"
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1]) and _same(res[0][2], res[1][2])


def test_a_separate_v_is_refused_by_both_binders():
    import flash_attn_2_cuda as ext
    kc = torch.zeros(2, 256, 1, D, device=DEV, dtype=BF)
    q = torch.zeros(2, 1, 16, D, device=DEV, dtype=BF)
    lens = torch.tensor([5, 9], dtype=torch.int32, device=DEV)
    sep = torch.zeros(2, 256, 1, DV, device=DEV, dtype=BF)
    for mod in (_be(), ext):
        with pytest.raises(RuntimeError, match=r"576, 512.*first 512 channels"):
            mod.fwd_kvcache(q, kc, sep, None, None, lens, None, None, None, None, None, None, None, SCALE, False, -1, -1, 0.0, True, 0)
        kn = torch.zeros(2, 1, 1, D, device=DEV, dtype=BF)
        with pytest.raises(RuntimeError, match=r"576, 512.*first 512 channels"):
            mod.fwd_kvcache(q, kc, kc[..., :DV], kn, torch.zeros(2, 1, 1, DV, device=DEV, dtype=BF), lens, None, None, None, None, None, None, None, SCALE, False,
                            -1, -1, 0.0, True, 0)


# ---- consistency ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 0, 3])
@pytest.mark.parametrize("shape", [_SHAPES[0], _SHAPES[3]], ids=lambda s: "H%d_Hk%d_Sq%d" % s[:3])
def test_addressings_agree_bit_for_bit(shape, splits):
    H, Hk, Sq, causal, window = shape
    q, kL = _problem(shape, BF)[:2]
    res = []
    for kind in ("contig", "idx", "paged256", "paged512"):
        g = torch.Generator().manual_seed(9)
        kc, idx, bt = _layout(kind, kL, _LENS, g, width=640 if kind == "idx" else D)   # (one of them with a free row stride)
        res.append(tuple(t.cpu() for t in _call(_be(), q, kc, torch.tensor(_LENS, dtype=torch.int32), idx, bt, causal, window, splits)))
        _assert_mla(BF, H // Hk)
    for o, l in res[1:]:
        assert _same(o, res[0][0]) and _same(l, res[0][1])


def test_binders_agree_and_repeats_are_bitwise_equal():
    import flash_attn_2_cuda as ext
    shape = _SHAPES[3]
    H, Hk, Sq, causal, window = shape
    q, kL = _problem(shape, BF)[:2]
    g = torch.Generator().manual_seed(3)
    kc, idx, bt = _layout("paged256", kL, _LENS, g)
    lens = torch.tensor(_LENS, dtype=torch.int32)
    for splits in (1, 0):
        first = tuple(t.cpu() for t in _call(_be(), q, kc, lens, idx, bt, causal, window, splits))
        _assert_mla(BF, H // Hk)
        o, l = _call(ext, q, kc, lens, idx, bt, causal, window, splits)
        _assert_mla(BF, H // Hk)
        assert _same(o.cpu(), first[0]) and _same(l.cpu(), first[1])
        for _ in range(10):
            o, l = _call(_be(), q, kc, lens, idx, bt, causal, window, splits)
            _assert_mla(BF, H // Hk)
            assert _same(o.cpu(), first[0]) and _same(l.cpu(), first[1])


def test_row_stride_640():
    shape = _SHAPES[2]
    ref = _problem(shape, BF)
    g = torch.Generator().manual_seed(4)
    kc, idx, bt = _layout("contig", ref[1], _LENS, g, width=640)
    assert kc.stride(1) == 640 and kc.shape[-1] == D
    out, lse = _call(_be(), ref[0], kc, torch.tensor(_LENS, dtype=torch.int32), idx, bt, False, (-1, -1), 0)
    _assert_mla(BF, 16)
    _check(out, lse, ref, "stride 640")
