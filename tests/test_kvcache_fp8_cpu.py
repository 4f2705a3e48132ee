"""CPU suite of the FP8 (e4m3) KV cache: exports, the validation of fa_fwd_kvcache_fp8 and of the fp8 fa_kvcache_append (they answer before
any launch, so no GPU is needed), both binders, the wrapper's Python checks and the split-KV workspace query."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8 = torch.float8_e4m3fn


def _lib():
    from flash_attn_amd import _cabi
    return _cabi, _cabi.load()


def _params(_cabi, **kw):
    a = _cabi.FaFwdParams()
    for n in ("q", "k", "v", "o", "softmax_lse"):
        setattr(a, n, C.c_void_p(4096))   # never dereferenced: every case below is answered before a launch
    a.b, a.h, a.h_k, a.d, a.seqlen_q, a.seqlen_k, a.total_q = 1, 8, 2, 128, 1, 8192, 1
    a.q_row_stride = a.o_row_stride = 8 * 128
    a.k_row_stride = a.v_row_stride = 2 * 128
    a.q_head_stride = a.k_head_stride = a.v_head_stride = a.o_head_stride = 128
    a.q_batch_stride = a.o_batch_stride = 8 * 128
    a.k_batch_stride = a.v_batch_stride = 8192 * 2 * 128
    a.dtype, a.softmax_scale = _cabi.FA_DTYPE_FP8_E4M3, 0.125
    for n, x in kw.items():
        setattr(a, n, x)
    return a


def _call(a, f=None):
    _cabi, lib = _lib()
    rc = lib.fa_fwd_kvcache_fp8(C.byref(a), C.byref(f) if f is not None else None, None)
    return rc, lib.fa_last_error().decode()


def test_exports_header_and_library_agree():
    _cabi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "fa_gfx950.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|void|const char\*)\s+(fa_\w+)\(", header, flags=re.M))
    assert "fa_fwd_kvcache_fp8" in declared
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    for n in declared:
        assert hasattr(lib, n), n
    assert lib.fa_abi_version() == _cabi.FA_ABI_VERSION == 6
    from flash_attn_amd import backend
    assert backend.FWD_KERNEL_NAMES[5] == "fa_fwd_fp8_kv_kernel"
    assert backend.FWD_KERNEL_NAMES[4] == "fa_fwd_fp8_kernel"


def test_kvcache_fp8_validates_before_any_launch():
    _cabi, _ = _lib()
    for dt in (_cabi.FA_DTYPE_BF16, _cabi.FA_DTYPE_FP16):
        rc, msg = _call(_params(_cabi, dtype=dt))
        assert rc == _cabi.FA_ERR_INVALID_ARGUMENT and "FA_DTYPE_FP8_E4M3" in msg
    unsupported = [
        (dict(d=96), "head dim 96"),
        (dict(d=256), "head dim 256"),
        (dict(softcap=30.0), "softcap"),
        (dict(alibi_slopes=C.c_void_p(4096)), "ALiBi"),
        (dict(leftpad_k=C.c_void_p(4096)), "leftpad"),
        (dict(p_dropout=0.1, rng_state=C.c_void_p(4096)), "dropout"),
        (dict(seqused_q=C.c_void_p(4096)), "seqused_q"),
    ]
    for kw, word in unsupported:
        rc, msg = _call(_params(_cabi, **kw), _cabi.FaFp8Params())
        assert rc == _cabi.FA_ERR_UNSUPPORTED and word in msg, (kw, rc, msg)
    invalid = [
        (dict(k_row_stride=2 * 128 + 8), "16 bytes"),
        (dict(q_head_stride=128 + 4), "16 bytes"),
        (dict(o_row_stride=8 * 128 + 4), "8 elements"),
        (dict(q=C.c_void_p(4096 + 8)), "16-byte aligned"),
        (dict(block_table=C.c_void_p(4096), page_block_size=100), "divisible by 256"),
        (dict(block_table=C.c_void_p(4096), page_block_size=256, cache_batch_idx=C.c_void_p(4096)), "cache_batch_idx"),
        (dict(cu_seqlens_q=C.c_void_p(4096), cu_seqlens_k=C.c_void_p(4096)), "cu_seqlens"),
        (dict(h=7), "Number of heads"),
    ]
    for kw, word in invalid:
        rc, msg = _call(_params(_cabi, **kw))
        assert rc == _cabi.FA_ERR_INVALID_ARGUMENT and word in msg, (kw, rc, msg)
    # forced splits without a workspace
    rc, msg = _call(_params(_cabi, num_splits=4))
    assert rc == _cabi.FA_ERR_WORKSPACE and "fa_fwd_workspace_bytes" in msg
    # the neighbours keep refusing what they refused: the prefill entry points take no cache arguments, the bf16 cache entry point no e4m3
    _, lib = _lib()
    for fn in (lib.fa_fwd_fp8, lib.fa_varlen_fwd_fp8):
        for kw in (dict(seqused_k=C.c_void_p(4096)), dict(cache_batch_idx=C.c_void_p(4096)), dict(num_splits=3),
                   dict(block_table=C.c_void_p(4096), page_block_size=256)):
            assert fn(C.byref(_params(_cabi, **kw)), None, None) == _cabi.FA_ERR_UNSUPPORTED, kw
    assert lib.fa_fwd_kvcache(C.byref(_params(_cabi)), None) == _cabi.FA_ERR_INVALID_ARGUMENT
    assert lib.fa_last_error().decode() == "FlashAttention only supports fp16 and bf16 data type"


def _append_params(_cabi, **kw):
    ap = _cabi.FaKvAppendParams()
    for n in ("knew", "vnew", "kcache", "vcache"):
        setattr(ap, n, C.c_void_p(4096))
    ap.knew_row_stride = ap.vnew_row_stride = ap.kcache_row_stride = ap.vcache_row_stride = 2 * 128
    ap.knew_head_stride = ap.vnew_head_stride = ap.kcache_head_stride = ap.vcache_head_stride = 128
    ap.knew_batch_stride = ap.vnew_batch_stride = 2 * 128
    ap.kcache_batch_stride = ap.vcache_batch_stride = 1024 * 2 * 128
    ap.b, ap.seqlen_new, ap.h_k, ap.d, ap.dtype = 1, 1, 2, 128, _cabi.FA_DTYPE_FP8_E4M3
    for n, x in kw.items():
        setattr(ap, n, x)
    return ap


def test_fp8_append_validates_before_any_launch():
    _cabi, lib = _lib()
    cases = [
        (dict(dtype=7), "fp16 and bf16"),
        (dict(d=72), "multiple of 16"),
        (dict(kcache_row_stride=2 * 128 + 8), "16 bytes"),
        (dict(knew_head_stride=128 + 8), "16 bytes"),
        (dict(vcache=C.c_void_p(4096 + 4)), "16-byte aligned"),
        (dict(block_table=C.c_void_p(4096), page_block_size=100), "divisible by 256"),
        (dict(block_table=C.c_void_p(4096), page_block_size=256, cache_batch_idx=C.c_void_p(4096)), "cache_batch_idx"),
    ]
    for kw, word in cases:
        rc = lib.fa_kvcache_append(C.byref(_append_params(_cabi, **kw)), None)
        assert rc == _cabi.FA_ERR_INVALID_ARGUMENT and word in lib.fa_last_error().decode(), (kw, rc, lib.fa_last_error())
    # nothing to copy: answered without a launch
    assert lib.fa_kvcache_append(C.byref(_append_params(_cabi, seqlen_new=0)), None) == _cabi.FA_OK
    # rotating quantised values is refused by name
    r = _cabi.FaRotaryParams()
    for n in ("x", "y", "cos", "sin"):
        setattr(r, n, C.c_void_p(4096))
    r.b, r.s, r.h, r.d, r.rotary_dim, r.seqlen_ro, r.dtype = 1, 1, 2, 128, 64, 16, _cabi.FA_DTYPE_FP8_E4M3
    assert lib.fa_rotary(C.byref(r), None) == _cabi.FA_ERR_UNSUPPORTED and "rotary" in lib.fa_last_error().decode()


def test_both_binders_expose_fwd_kvcache_fp8_and_refuse_cpu_tensors():
    import flash_attn_2_cuda as ext
    from flash_attn_amd import backend
    q = torch.zeros(1, 1, 4, 64, dtype=FP8)
    kc = torch.zeros(1, 256, 2, 64, dtype=FP8)
    for m in (ext, backend):
        assert callable(m.fwd_kvcache_fp8)
        with pytest.raises(RuntimeError, match="CUDA"):
            m.fwd_kvcache_fp8(q, kc, kc, None, None, None, None, None, None, None, None, None, 0.125, False, -1, -1, 0)


def test_wrapper_checks_run_before_the_backend():
    """On CPU tensors: had a call reached the backend it would have raised the device error instead."""
    from flash_attn_amd import flash_attn_with_kvcache
    q = torch.zeros(2, 1, 8, 64, dtype=FP8)
    kc = torch.zeros(2, 256, 2, 64, dtype=FP8)
    qb, kb = q.to(torch.bfloat16), kc.to(torch.bfloat16)
    ds = torch.ones(2, 2)
    with pytest.raises(RuntimeError, match=r"k_descale must have shape \(batch_size, num_heads_k\) = \(2, 2\)"):
        flash_attn_with_kvcache(q, kc, kc, k_descale=torch.ones(2, 8))
    with pytest.raises(RuntimeError, match="v_descale must have shape"):
        flash_attn_with_kvcache(q, kc, kc, v_descale=torch.ones(2))
    with pytest.raises(RuntimeError, match="float8_e4m3fn inputs only"):
        flash_attn_with_kvcache(qb, kb, kb, q_descale=ds)
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        flash_attn_with_kvcache(qb, kc, kc)
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        flash_attn_with_kvcache(q, kc, kb)
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        flash_attn_with_kvcache(q, kc, kc, k=torch.zeros(2, 1, 2, 64, dtype=torch.bfloat16), v=torch.zeros(2, 1, 2, 64, dtype=FP8), cache_seqlens=3)
    cos = torch.zeros(256, 16)
    with pytest.raises(RuntimeError, match="rotary"):
        flash_attn_with_kvcache(q, kc, kc, rotary_cos=cos, rotary_sin=cos)
    with pytest.raises(RuntimeError, match="cache_leftpad"):
        flash_attn_with_kvcache(q, kc, kc, cache_leftpad=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="softcap"):
        flash_attn_with_kvcache(q, kc, kc, softcap=30.0)
    with pytest.raises(RuntimeError, match="ALiBi"):
        flash_attn_with_kvcache(q, kc, kc, alibi_slopes=torch.ones(8))
    with pytest.raises(RuntimeError, match="CUDA"):   # a valid call gets through the wrapper's checks and meets the binder's device check
        flash_attn_with_kvcache(q, kc, kc, q_descale=ds, k_descale=ds, v_descale=ds)


def test_workspace_bytes_answer_for_an_fp8_decode():
    _cabi, lib = _lib()
    a = _params(_cabi)   # B = 1, Sk = 8192, H = 8 / 2, one query row
    n = lib.fa_fwd_workspace_bytes(C.byref(a))
    assert n > 0 and n % ((128 + 1) * 4 * 8) == 0   # whole partial rows (fp32 o of pitch 128 + the lse) of the 8 query heads
    assert lib.fa_fwd_workspace_bytes(C.byref(_params(_cabi, num_splits=1))) == 0
    assert lib.fa_fwd_workspace_bytes(C.byref(_params(_cabi, num_splits=4))) == 4 * 8 * (128 + 1) * 4
    assert lib.fa_fwd_workspace_bytes(C.byref(_params(_cabi, seqlen_q=300, total_q=300))) == 0   # a long chunk runs unsplit
