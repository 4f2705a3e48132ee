"""Round 7 changed the once-per-block code of the 64-rows-per-wave forward (fa_fwd_w64.hip): the block decode divides by multiply-shift reciprocals, a fixed-length
batch without a left window takes a DENSE instantiation with the per-block array tests, left limits and two-sided ranges compiled out, and a masked iteration
followed by the wave's peeled last one no longer restores the mask broadcasts.  The cases are the smallest shapes at which each piece can go wrong; every one is
pinned to the kernel (FA_FWD_NW=64) and judged like the w64 cases of tests/test_fwd_gpu.py: against the fp64 oracle, |out - ref| < max(2 x the lock-step kernel's
error, 1.2e-2 bf16 / 4e-3 fp16), |lse - ref| < 8e-3 bf16 / 2e-3 fp16, +inf exactly on the rows that see no key."""
import numpy as np
import pytest
import torch

from tests._dropout_model import threshold as dropout_threshold
from tests._util import max_abs
from tests.test_w64_dirty_registers_gpu import dirty

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16


@pytest.fixture(scope="module")
def be():
    from flash_attn_amd import backend
    return backend


def _qkv(B, Sq, Sk, H, Hk, D, dtype, seed):
    torch.manual_seed(seed)
    q = torch.randn(B, Sq, H, D, device="cuda", dtype=dtype)
    k = torch.randn(B, Sk, Hk, D, device="cuda", dtype=dtype)
    return q, k, torch.randn_like(k)


def _is_w64(s, variant):
    """last_schedule() names the instantiation: "...,dense>" for the dense one, "<T,D>" for the general plain one, "...,alibi>" etc. for the features."""
    want = {"dense": ",dense>", "general": None, "alibi": ",alibi>", "softcap": ",softcap>", "dropout": ",dropout>", "paged": ",paged>"}[variant]
    ok = s["name"].endswith(want) if want else s["name"].count(",") == 1
    return s["fwd_kernel"] == 3 and s["name"].startswith("fa::fa_fwd_w64_kernel<") and ok


def _pair(be, knobs, run, variant):
    """run() on the 64-rows-per-wave kernel (the named instantiation) and on the lock-step kernel."""
    knobs.set("FA_FWD_NW", "64")
    out, lse = run()
    s = be.last_schedule()
    assert _is_w64(s, variant), (variant, s)
    knobs.set("FA_FWD_NW", "8")
    out8, _ = run()
    assert be.last_schedule()["fwd_kernel"] == 1
    knobs.unset("FA_FWD_NW")
    return out, lse, out8


def _judge(out, lse, out8, ref, lse_ref, dtype, scale=1.0):
    ref, lse_ref = torch.from_numpy(ref).float(), torch.from_numpy(lse_ref).float()
    assert torch.isfinite(out.float()).all()
    e64, e8 = max_abs(out.float().cpu(), ref), max_abs(out8.float().cpu(), ref)
    fin = torch.isfinite(lse_ref)
    el = max_abs(lse.cpu()[fin], lse_ref[fin])
    print(f"e64={e64:.3e} e8={e8:.3e} el={el:.3e}")
    assert e64 < max(2 * e8, (1.2e-2 if dtype == BF16 else 4e-3) * scale), (e64, e8)
    assert torch.equal(torch.isposinf(lse.cpu()), ~fin)
    assert el < (8e-3 if dtype == BF16 else 2e-3), el


def _plain(be, knobs, B, Sq, Sk, H, Hk, D, dtype, causal, window=(-1, -1), seed=0):
    from oracle import attention_oracle as orc
    q, k, v = _qkv(B, Sq, Sk, H, Hk, D, dtype, seed)
    run = lambda: be.fwd(q, k, v, None, None, 0.0, D ** -0.5, causal, window[0], window[1], 0.0, False, None)[:2]
    out, lse, out8 = _pair(be, knobs, run, "dense" if window[0] < 0 else "general")
    ref, lse_ref = orc.attention_fwd(q, k, v, D ** -0.5, causal, window)
    _judge(out, lse, out8, ref, lse_ref, dtype)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("d,dtype", [(128, BF16), (64, BF16), (128, FP16), (64, FP16)], ids=["d128-bf16", "d64-bf16", "d128-fp16", "d64-fp16"])
def test_persistent_walk_reaches_a_second_mirrored_round(be, knobs, d, dtype, causal):
    """B2 H80 S512: 320 blocks for 256 workgroups -- the decode of a second round, mirrored inside its units under the causal mask, on the dense variant."""
    _plain(be, knobs, 2, 512, 512, 80, 80, d, dtype, causal, seed=d + causal)


def test_grouped_heads_divide_by_hk_ratio(be, knobs):
    _plain(be, knobs, 2, 512, 512, 80, 20, 128, BF16, True, seed=3)


def test_partial_last_block_with_waves_that_own_no_row(be, knobs):
    """S = 600: block 2 has 88 rows -- wave 1 partial, waves 2 and 3 without rows."""
    _plain(be, knobs, 2, 600, 600, 4, 2, 128, BF16, True, seed=4)
    _plain(be, knobs, 2, 600, 600, 4, 2, 128, BF16, False, seed=5)


@pytest.mark.parametrize("sk", [552, 576])
def test_causal_diagonal_off_the_tile_grid(be, knobs, sk):
    """shift = 40 (the diagonal cuts through the 32-key steps: set_mask element by element) and shift = 64 (tile-aligned but shifted); the masked iteration is followed by
    the wave's last one, whose skipped clear_mask must not be missed."""
    _plain(be, knobs, 2, 512, sk, 4, 2, 128, BF16, True, seed=sk)


@pytest.mark.parametrize("window", [(64, 0), (100, 30)])
def test_left_windows_keep_their_clear_mask(be, knobs, window):
    """The non-dense path: masked iterations at the left edge are followed by plain ones."""
    _plain(be, knobs, 1, 768, 768, 4, 2, 128, BF16, False, window, seed=7 + window[0])
    _plain(be, knobs, 1, 768, 768, 4, 4, 64, FP16, False, window, seed=8 + window[0])


@pytest.mark.parametrize("seqused", [False, True], ids=["cu_seqlens", "cu_seqlens+seqused_k"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_packed_batch_equals_the_dense_variant_bit_for_bit(be, knobs, causal, seqused):
    """Three sequences of 512 as a cu_seqlens batch (the general instantiation) against the fixed-length call on each (the dense one): the same bits."""
    torch.manual_seed(11)
    H, Hk, D, S, B = 8, 2, 128, 512, 3
    q = torch.randn(B * S, H, D, device="cuda", dtype=BF16)
    k = torch.randn(B * S, Hk, D, device="cuda", dtype=BF16)
    v = torch.randn_like(k)
    cu = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device="cuda")
    used = torch.full((B,), S, dtype=torch.int32, device="cuda") if seqused else None
    knobs.set("FA_FWD_NW", "64")
    out, lse = be.varlen_fwd(q, k, v, None, cu, cu, used, None, None, None, S, S, 0.0, D ** -0.5, False, causal, -1, -1, 0.0, False, None)[:2]
    assert _is_w64(be.last_schedule(), "general"), be.last_schedule()
    for b in range(B):
        sl = slice(b * S, (b + 1) * S)
        o1, l1 = be.fwd(q[None, sl], k[None, sl], v[None, sl], None, None, 0.0, D ** -0.5, causal, -1, -1, 0.0, False, None)[:2]
        assert _is_w64(be.last_schedule(), "dense"), be.last_schedule()
        assert torch.equal(out[sl], o1[0]) and torch.equal(lse[:, sl], l1[0]), b
    knobs.unset("FA_FWD_NW")


def test_feature_variants_share_the_edited_prologue_and_epilogue(be, knobs):
    """Causal ALiBi, softcap, dropout and the paged variant at B1 H4 S768."""
    from oracle import attention_oracle as orc
    B, S, H, Hk, D = 1, 768, 4, 2, 128
    sc = D ** -0.5
    q, k, v = _qkv(B, S, S, H, Hk, D, BF16, 21)
    slopes = torch.tensor([0.5, 0.25, 0.0625, 0.0078125], device="cuda", dtype=torch.float32)
    out, lse, out8 = _pair(be, knobs, lambda: be.fwd(q, k, v, None, slopes, 0.0, sc, True, -1, -1, 0.0, False, None)[:2], "alibi")
    _judge(out, lse, out8, *orc.attention_fwd(q, k, v, sc, True, (-1, -1), 0.0, slopes.cpu().numpy()), BF16)
    out, lse, out8 = _pair(be, knobs, lambda: be.fwd(q, k, v, None, None, 0.0, sc, True, -1, -1, 30.0, False, None)[:2], "softcap")
    _judge(out, lse, out8, *orc.attention_fwd(q, k, v, sc, True, (-1, -1), 30.0, None), BF16)
    # dropout: the mask from the lock-step kernel's random bytes under the same seed
    p = 0.2
    knobs.set("FA_FWD_NW", "8")
    torch.manual_seed(77)
    out8, _, rv, rng8 = be.fwd(q, k, v, None, None, p, sc, True, -1, -1, 0.0, True, None)
    assert be.last_schedule()["fwd_kernel"] == 1
    knobs.set("FA_FWD_NW", "64")
    torch.manual_seed(77)
    out, lse, _, rng = be.fwd(q, k, v, None, None, p, sc, True, -1, -1, 0.0, False, None)
    s = be.last_schedule()
    knobs.unset("FA_FWD_NW")
    assert _is_w64(s, "dropout"), s
    assert torch.equal(rng, rng8)
    keep = (rv.to(torch.int32) <= dropout_threshold(p)).cpu().numpy()
    _judge(out, lse, out8, *orc.attention_fwd(q, k, v, sc, True, (-1, -1), 0.0, None, p, keep), BF16, 1.0 / (1.0 - p))
    # paged: the same keys and values in shuffled pages of 256
    page, per = 256, S // 256
    table = torch.tensor([[2, 0, 3]], dtype=torch.int32, device="cuda")
    kp = torch.randn(per + 1, page, Hk, D, device="cuda", dtype=BF16)
    vp = torch.randn_like(kp)
    kp[table[0].long()] = k[0].reshape(per, page, Hk, D); vp[table[0].long()] = v[0].reshape(per, page, Hk, D)
    cu = torch.tensor([0, S], dtype=torch.int32, device="cuda")
    run = lambda: be.varlen_fwd(q[0], kp, vp, None, cu, cu, None, None, table, None, S, S, 0.0, sc, False, True, -1, -1, 0.0, False, None)[:2]
    out, lse, out8 = _pair(be, knobs, run, "paged")
    ref, lse_ref = orc.attention_fwd(q, k, v, sc, True)
    _judge(out[None], lse[None], out8[None], ref, lse_ref, BF16)


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("window", [(-1, 0), (200, 0)], ids=["dense", "general"])
def test_plain_instantiations_after_dirty_registers(be, knobs, window, dtype, d):
    """The probe of tests/test_w64_dirty_registers_gpu.py for both plain instantiations: the dense one (a right bound alone) and the general one (a left window)."""
    torch.manual_seed(0)
    q = torch.randn(2, 1536, 8, d, device="cuda", dtype=dtype)
    k, v = torch.randn_like(q), torch.randn_like(q)
    res = []
    for kind in (0, 1):
        dirty(be, knobs, kind, dtype)
        knobs.set("FA_FWD_NW", 64)
        o, lse, _, _ = be.fwd(q, k, v, None, None, 0.0, d ** -0.5, False, window[0], window[1], 0.0, False, None)
        assert _is_w64(be.last_schedule(), "dense" if window[0] < 0 else "general"), be.last_schedule()
        res.append((o.clone(), lse.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.isfinite(res[0][0].float()).all()
