"""CPU suite of the absorbed MLA decode pair (q / k head dim 576, v / o head dim 512, v_cache = k_cache[..., :512]): the C ABI's validation, the
workspace query, every refusal of the contract by message -- in the C ABI and through the public functions on CPU tensors --, the kernel table and the
static resources of the new kernel family.  Every case is answered before a launch."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.test_kernel_resources_cpu import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, DV = 576, 512
BF = torch.bfloat16


def _lib():
    from flash_attn_amd import _cabi
    return _cabi, _cabi.load()


def _fwd_params(_cabi, **kw):
    a = _cabi.FaFwdParams()
    for n in ("q", "k", "v", "o", "softmax_lse"):
        setattr(a, n, C.c_void_p(4096))   # never dereferenced: every case below is answered before a launch (k == v: the latent view)
    a.b, a.h, a.h_k, a.d, a.d_v, a.seqlen_q, a.seqlen_k, a.total_q = 2, 16, 1, D, DV, 1, 1024, 2
    a.q_batch_stride, a.q_row_stride, a.q_head_stride = 16 * D, 16 * D, D
    a.o_batch_stride, a.o_row_stride, a.o_head_stride = 16 * DV, 16 * DV, DV
    for n in ("k", "v"):
        setattr(a, n + "_batch_stride", 1024 * D); setattr(a, n + "_row_stride", D); setattr(a, n + "_head_stride", D)
    a.dtype, a.softmax_scale, a.window_left, a.window_right = _cabi.FA_DTYPE_BF16, D ** -0.5, -1, -1
    for n, x in kw.items():
        setattr(a, n, x)
    return a


def _bwd_params(_cabi, **kw):
    a = _cabi.FaBwdParams()
    a.b, a.h, a.h_k, a.d, a.d_v, a.seqlen_q, a.seqlen_k, a.total_q, a.total_k = 2, 16, 1, D, DV, 256, 256, 512, 512
    a.dtype, a.softmax_scale, a.window_left, a.window_right = _cabi.FA_DTYPE_BF16, D ** -0.5, -1, -1
    for n, x in kw.items():
        setattr(a, n, x)
    return a


def _err(lib):
    return lib.fa_last_error().decode()


# ---------------------------------------------------------------- C ABI: validation
def test_the_latent_view_passes_validation():
    _cabi, lib = _lib()
    # stops at the first pointer check ...
    assert lib.fa_fwd_kvcache(C.byref(_fwd_params(_cabi, q=None)), None) == _cabi.FA_ERR_INVALID_ARGUMENT and "non-NULL" in _err(lib)
    # ... or has nothing to write
    assert lib.fa_fwd_kvcache(C.byref(_fwd_params(_cabi, seqlen_q=0, total_q=0)), None) == _cabi.FA_OK
    # the cache arguments, masks, a paged cache and split keys belong to the contract: still the pointer check
    ptr = C.c_void_p(4096)
    for kw in (dict(seqused_k=ptr, cache_batch_idx=ptr), dict(seqused_k=ptr, block_table=ptr, page_block_size=256, block_table_batch_stride=4),
               dict(is_causal=1, seqlen_q=5, total_q=10), dict(window_left=100, window_right=0), dict(num_splits=3), dict(dtype=_cabi.FA_DTYPE_FP16),
               dict(k_row_stride=640, v_row_stride=640, k_batch_stride=640 * 1024, v_batch_stride=640 * 1024), dict(h=8, h_k=2), dict(h=4, h_k=4)):
        rc = lib.fa_fwd_kvcache(C.byref(_fwd_params(_cabi, q=None, **kw)), None)
        assert rc == _cabi.FA_ERR_INVALID_ARGUMENT and "non-NULL" in _err(lib), (kw, rc, _err(lib))


def test_a_separate_v_is_refused_by_name():
    _cabi, lib = _lib()
    for kw in (dict(v=C.c_void_p(8192)), dict(v_row_stride=DV), dict(v_head_stride=DV), dict(v_batch_stride=1024 * DV)):
        rc = lib.fa_fwd_kvcache(C.byref(_fwd_params(_cabi, **kw)), None)
        assert rc == _cabi.FA_ERR_UNSUPPORTED and re.search(r"576, 512.*V must be the first 512 channels of K", _err(lib)), (kw, rc, _err(lib))


def test_strides_and_alignment_are_checked_before_the_launch():
    _cabi, lib = _lib()
    for kw in (dict(k_row_stride=580, v_row_stride=580), dict(k_row_stride=512, v_row_stride=512), dict(q_row_stride=16 * D + 4), dict(o_head_stride=DV + 2),
               dict(q=C.c_void_p(4100)), dict(k=C.c_void_p(4104), v=C.c_void_p(4104))):
        rc = lib.fa_fwd_kvcache(C.byref(_fwd_params(_cabi, **kw)), None)
        assert rc == _cabi.FA_ERR_INVALID_ARGUMENT and re.search(r"576, 512.*(strides|aligned)", _err(lib)), (kw, rc, _err(lib))


def test_workspace_is_sized_at_the_value_width():
    _cabi, lib = _lib()
    a = _fwd_params(_cabi, b=1, h=128, h_k=1, seqlen_q=1, seqlen_k=8192, total_q=1, num_splits=4)
    assert lib.fa_fwd_workspace_bytes(C.byref(a)) == 4 * 128 * 513 * 4
    a.num_splits = 1
    assert lib.fa_fwd_workspace_bytes(C.byref(a)) == 0
    # the heuristic: one workgroup per CU -- 2 blocks of 64 rows for this shape, so at most 128 splits, at least 4 tiles each: 32
    a.num_splits = 0
    assert lib.fa_fwd_workspace_bytes(C.byref(a)) == 32 * 128 * 513 * 4
    # keys are split only while the packed rows fit 128 (as every other kernel's rule)
    a.seqlen_q, a.total_q, a.num_splits = 2, 2, 4
    assert lib.fa_fwd_workspace_bytes(C.byref(a)) == 0
    # a forced split without the workspace is an error of its own, not a launch
    a = _fwd_params(_cabi, num_splits=4)
    assert lib.fa_fwd_kvcache(C.byref(a), None) == _cabi.FA_ERR_WORKSPACE


# ---------------------------------------------------------------- C ABI: refusals
def test_refusals_of_the_c_abi_name_the_pair_or_the_argument():
    _cabi, lib = _lib()
    ptr = C.c_void_p(4096)
    cases = [
        (lib.fa_fwd_kvcache, dict(leftpad_k=ptr, seqused_k=ptr), r"576, 512.*leftpad_k"),
        (lib.fa_fwd_kvcache, dict(alibi_slopes=ptr), r"576, 512.*ALiBi"),
        (lib.fa_fwd_kvcache, dict(softcap=30.0), r"576, 512.*softcap"),
        (lib.fa_fwd, dict(seqlen_q=256, seqlen_k=256, total_q=512), r"fa_fwd: head dims \(576, 512\).*fa_fwd_kvcache only"),
        (lib.fa_varlen_fwd, dict(cu_seqlens_q=ptr, cu_seqlens_k=ptr), r"fa_varlen_fwd: head dims \(576, 512\).*fa_fwd_kvcache only"),
        # every other new pair: the answers the parent gave
        (lib.fa_fwd_kvcache, dict(d=128, d_v=512), r"128, 512.*KV-cache path has no kernel"),
        (lib.fa_fwd_kvcache, dict(d=64, d_v=512), r"64, 512.*KV-cache path has no kernel"),
        (lib.fa_fwd_kvcache, dict(d=192, d_v=128), r"192, 128.*KV-cache path has no kernel"),
        (lib.fa_fwd, dict(d=256, d_v=512), r"256, 512.*only built pair"),
    ]
    for fn, kw, pat in cases:
        rc = fn(C.byref(_fwd_params(_cabi, **kw)), None)
        assert rc == _cabi.FA_ERR_UNSUPPORTED and re.search(pat, _err(lib)), (kw, rc, _err(lib))
    assert lib.fa_fwd_schedule_query(C.byref(_fwd_params(_cabi)), 0) == _cabi.FA_ERR_UNSUPPORTED and re.search(r"576, 512", _err(lib))
    # the fp8 entry points
    for fn in (lib.fa_fwd_fp8, lib.fa_varlen_fwd_fp8, lib.fa_fwd_kvcache_fp8):
        rc = fn(C.byref(_fwd_params(_cabi, dtype=_cabi.FA_DTYPE_FP8_E4M3)), None, None)
        assert rc == _cabi.FA_ERR_UNSUPPORTED and re.search(r"576, 512.*fp8", _err(lib)), (rc, _err(lib))
    # the backward
    for fn, kw in ((lib.fa_bwd, dict()), (lib.fa_varlen_bwd, dict(cu_seqlens_q=ptr, cu_seqlens_k=ptr))):
        rc = fn(C.byref(_bwd_params(_cabi, **kw)), None)
        assert rc == _cabi.FA_ERR_UNSUPPORTED and re.search(r"bwd: head dims \(576, 512\).*no backward", _err(lib)), (rc, _err(lib))
    assert lib.fa_bwd_dq_schedule_query(C.byref(_bwd_params(_cabi))) == _cabi.FA_ERR_UNSUPPORTED
    # head dim 576 without the value width 512: the "at most 256" answer stays
    for fn, dv in ((lib.fa_fwd_kvcache, 0), (lib.fa_fwd_kvcache, 576), (lib.fa_fwd, 0), (lib.fa_fwd_kvcache, 128), (lib.fa_fwd_kvcache, 256)):
        rc = fn(C.byref(_fwd_params(_cabi, d_v=dv)), None)
        assert rc == _cabi.FA_ERR_INVALID_ARGUMENT and "at most 256" in _err(lib), (dv, rc, _err(lib))
    assert lib.fa_bwd(C.byref(_bwd_params(_cabi, d_v=0)), None) == _cabi.FA_ERR_INVALID_ARGUMENT and "at most 256" in _err(lib)


# ---------------------------------------------------------------- the public functions, on CPU tensors
def _tensors(B=2, Sq=1, H=16, Hk=1, Sk=256):
    return torch.zeros(B, Sq, H, D, dtype=BF), torch.zeros(B, Sk, Hk, D, dtype=BF)


def test_public_refusals_on_cpu_tensors():
    from flash_attn_amd import flash_attn_interface as fi
    q, kc = _tensors()
    v = kc[..., :DV]
    kn = torch.zeros(2, 1, 1, D, dtype=BF)
    rc, rs = torch.zeros(256, 32, dtype=BF), torch.zeros(256, 32, dtype=BF)
    i32 = torch.zeros(2, dtype=torch.int32)
    cu = torch.zeros(3, dtype=torch.int32)
    f8 = torch.float8_e4m3fn
    cases = [
        (lambda: fi.flash_attn_with_kvcache(q, kc, v, k=kn, rotary_cos=rc, rotary_sin=rs, cache_seqlens=5), r"576, 512.*rotary"),
        (lambda: fi.flash_attn_with_kvcache(q, kc, v, cache_seqlens=5, cache_leftpad=i32), r"576, 512.*cache_leftpad"),
        (lambda: fi.flash_attn_with_kvcache(q, kc, v, cache_seqlens=5, alibi_slopes=torch.zeros(16)), r"576, 512.*alibi_slopes"),
        (lambda: fi.flash_attn_with_kvcache(q, kc, v, cache_seqlens=5, softcap=30.0), r"576, 512.*softcap"),
        (lambda: fi.flash_attn_with_kvcache(q, kc, v, cache_seqlens=5, q_descale=torch.ones(2, 1)), r"576, 512.*fp8"),
        (lambda: fi.flash_attn_with_kvcache(q.to(f8), kc.to(f8), kc.to(f8)[..., :DV], cache_seqlens=5), r"576, 512.*fp8"),
        # V must be the latent part of the same memory
        (lambda: fi.flash_attn_with_kvcache(q, kc, torch.zeros(2, 256, 1, DV, dtype=BF), cache_seqlens=5), r"576, 512.*v_cache must be the first 512 channels of k_cache"),
        (lambda: fi.flash_attn_with_kvcache(q, kc, kc[..., 64:], cache_seqlens=5), r"576, 512.*v_cache must be the first 512 channels of k_cache"),
        (lambda: fi.flash_attn_with_kvcache(q, kc, kc[:, :, :, :DV].clone(), cache_seqlens=5), r"576, 512.*v_cache must be the first 512 channels of k_cache"),
        (lambda: fi.flash_attn_with_kvcache(q, kc, v, k=kn, v=torch.zeros(2, 1, 1, DV, dtype=BF), cache_seqlens=5), r"576, 512.*v must be None or the first 512 channels of k"),
        # the other entry points
        (lambda: fi.flash_attn_func(q, kc, v), r"flash_attn_func.*576, 512"),
        (lambda: fi.flash_attn_func(q.requires_grad_(False), kc, v, causal=True), r"576, 512"),
        (lambda: fi.flash_attn_varlen_func(q[:, 0], kc[:, 0], v[:, 0], cu, cu, 1, 1), r"flash_attn_varlen_func.*576, 512"),
        (lambda: fi.flash_attn_padded_func(q, kc, v, i32, i32), r"flash_attn_padded_func.*576, 512"),
        # every other new pair / 576 alone
        (lambda: fi.flash_attn_with_kvcache(q, kc, kc[..., :256], cache_seqlens=5), r"576, 256.*KV-cache path has no kernel"),
        (lambda: fi.flash_attn_with_kvcache(q[..., :128], kc[..., :128], v, cache_seqlens=5), r"128, 512.*KV-cache path has no kernel"),
    ]
    for fn, pat in cases:
        with pytest.raises(RuntimeError, match=pat):
            fn()
    # valid calls get as far as the binder's device check
    for kw in (dict(), dict(k=kn), dict(k=kn, v=kn[..., :DV]), dict(causal=True, window_size=(64, 0), num_splits=3),
               dict(block_table=torch.zeros(2, 1, dtype=torch.int32)), dict(cache_batch_idx=i32)):
        with pytest.raises(RuntimeError, match="CUDA"):
            fi.flash_attn_with_kvcache(q, kc, v, cache_seqlens=i32, **kw)
    q2, kc2 = (t.to(torch.float16) for t in _tensors(H=8, Hk=2))
    with pytest.raises(RuntimeError, match="CUDA"):
        fi.flash_attn_with_kvcache(q2, kc2, kc2[..., :DV], cache_seqlens=7)


def test_the_ctypes_binder_refuses_the_same():
    from flash_attn_amd import backend as be
    assert be.FWD_KERNEL_NAMES[7] == "fa_fwd_mla_kernel" and be.MLA_DECODE_PAIR == (576, 512) and be.HEAD_DIM_PAIRS == ((192, 128),)
    for kw, pat in ((dict(rotary=True), r"576, 512.*rotary"), (dict(leftpad_k=True), r"576, 512.*leftpad_k"), (dict(alibi_slopes=True), r"576, 512.*ALiBi"),
                    (dict(softcap=1.0), r"576, 512.*softcap")):
        with pytest.raises(RuntimeError, match=pat):
            be.check_mla_decode("fwd_kvcache", **kw)
    be.check_mla_decode("fwd_kvcache")
    q, kc = _tensors()
    assert be.is_latent_view(kc[..., :DV], kc) and not be.is_latent_view(kc[..., 64:], kc) and not be.is_latent_view(kc[..., :DV].clone(), kc)
    assert not be.is_latent_view(kc[:1, :, :, :DV], kc) and not be.is_latent_view(kc[..., :256], kc)
    with pytest.raises(RuntimeError, match=r"576, 512.*only built pair"):
        be.check_head_dim_pair("fwd", D, DV)


def test_header_and_exports_are_unchanged():
    _cabi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "fa_gfx950.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|void|const char\*)\s+(fa_\w+)\(", header, flags=re.M))
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    assert re.search(r"#define FA_SCHEDULE_FIELDS 13\b", header) and re.search(r"#define FA_ABI_VERSION 6\b", header)
    assert "7 fa_fwd_mla_kernel" in header and "k_cache[..., :512]" in header
    assert lib.fa_sizeof_fwd_params() == C.sizeof(_cabi.FaFwdParams) == 344 and lib.fa_sizeof_kvappend_params() == C.sizeof(_cabi.FaKvAppendParams)


# ---------------------------------------------------------------- static resources
def test_the_new_family_has_two_kernels_without_scratch():
    ks = kernel_metadata()
    fam = {n: v for n, v in ks.items() if "fa_fwd_mla_kernel" in n}
    assert len(fam) == 2, sorted(fam)   # bf16 and fp16, <E, 576, 512, 4 waves>
    for n, v in fam.items():
        assert re.findall(r"Li(\d+)E", n) == ["576", "512", "4"], n
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (n, v)
    # the name must not be counted into another family of tests/test_kernel_resources_cpu.py
    for other in ("fa_fwd_kernel", "fa_fwd_dv_kernel", "fa_fwd_fp8_kernel", "fa_fwd_fp8_kv_kernel"):
        assert not any(other in n for n in fam)
    # the merge of its fp32 partials, at the value width
    assert sum("fa_splitkv_combine_kernel" in n and re.findall(r"Li(\d+)E", n) == ["512", "512"] for n in ks) == 2
