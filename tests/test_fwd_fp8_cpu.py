"""CPU suite of the FP8 (e4m3) forward: exports and the C-ABI mirror, the validation of fa_fwd_fp8 / fa_varlen_fwd_fp8 (it answers before
any launch, so no GPU is needed), the custom ops and their fakes, the wrapper's checks under fake tensors, and the MFMA pricing of the
hazard check for the block-scaled instruction the fp8 kernel issues."""
import ctypes as C
import importlib.util
import os

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8 = torch.float8_e4m3fn


def _lib():
    from flash_attn_amd import _cabi
    return _cabi, _cabi.load()


def _params(_cabi, **kw):
    a = _cabi.FaFwdParams()
    for n in ("q", "k", "v", "o", "softmax_lse"):
        setattr(a, n, C.c_void_p(4096))   # never dereferenced: every case below is refused before a launch
    a.b, a.h, a.h_k, a.d, a.seqlen_q, a.seqlen_k, a.total_q = 1, 4, 2, 128, 64, 64, 64
    a.q_row_stride = a.k_row_stride = a.v_row_stride = 4 * 128
    a.q_head_stride = a.k_head_stride = a.v_head_stride = a.o_head_stride = 128
    a.o_row_stride = 4 * 128
    a.q_batch_stride = a.k_batch_stride = a.v_batch_stride = a.o_batch_stride = 64 * 4 * 128
    a.dtype, a.softmax_scale = _cabi.FA_DTYPE_FP8_E4M3, 0.125
    for n, x in kw.items():
        setattr(a, n, x)
    return a


def _call(fn, a, f=None):
    _cabi, lib = _lib()
    rc = getattr(lib, fn)(C.byref(a), C.byref(f) if f is not None else None, None)
    return rc, lib.fa_last_error().decode()


def test_fp8_exports_and_struct_mirror():
    _cabi, lib = _lib()
    for n in ("fa_fwd_fp8", "fa_varlen_fwd_fp8", "fa_sizeof_fp8_params"):
        assert n in _cabi.EXPORTS and hasattr(lib, n)
    assert lib.fa_sizeof_fp8_params() == C.sizeof(_cabi.FaFp8Params) == 3 * 8 + 6 * 8
    assert _cabi.FA_DTYPE_FP8_E4M3 == 2 and lib.fa_sizeof_fwd_params() == C.sizeof(_cabi.FaFwdParams)
    from flash_attn_amd import backend
    assert backend.FWD_KERNEL_NAMES[4] == "fa_fwd_fp8_kernel"


def test_fp8_entry_points_validate_before_any_launch():
    _cabi, _ = _lib()
    rc, msg = _call("fa_fwd_fp8", _params(_cabi, dtype=_cabi.FA_DTYPE_BF16))
    assert rc == _cabi.FA_ERR_INVALID_ARGUMENT and "FA_DTYPE_FP8_E4M3" in msg
    unsupported = [
        (dict(d=96), "head dim 96"),
        (dict(softcap=30.0), "softcap"),
        (dict(alibi_slopes=C.c_void_p(4096)), "ALiBi"),
        (dict(p_dropout=0.1, rng_state=C.c_void_p(4096)), "dropout"),
        (dict(randval=C.c_void_p(4096)), "return_softmax"),
        (dict(block_table=C.c_void_p(4096), page_block_size=256), "block_table"),
        (dict(seqused_k=C.c_void_p(4096)), "seqused"),
        (dict(seqused_q=C.c_void_p(4096)), "seqused"),
        (dict(leftpad_k=C.c_void_p(4096)), "leftpad_k"),
        (dict(cache_batch_idx=C.c_void_p(4096)), "KV-cache"),
    ]
    for kw, word in unsupported:
        for fn in ("fa_fwd_fp8", "fa_varlen_fwd_fp8"):
            rc, msg = _call(fn, _params(_cabi, **kw), _cabi.FaFp8Params())
            assert rc == _cabi.FA_ERR_UNSUPPORTED and word in msg, (fn, kw, rc, msg)
    # the contract's layout rules: e4m3 strides in 16-byte units, cu_seqlens consistent with the entry point
    rc, msg = _call("fa_fwd_fp8", _params(_cabi, q_row_stride=4 * 128 + 8))
    assert rc == _cabi.FA_ERR_INVALID_ARGUMENT and "16 bytes" in msg
    rc, msg = _call("fa_varlen_fwd_fp8", _params(_cabi))
    assert rc == _cabi.FA_ERR_INVALID_ARGUMENT and "cu_seqlens" in msg
    # the bf16 / fp16 entry points keep refusing the fp8 dtype with their message
    _, lib = _lib()
    for fn in (lib.fa_fwd, lib.fa_varlen_fwd):
        assert fn(C.byref(_params(_cabi)), None) == _cabi.FA_ERR_INVALID_ARGUMENT
        assert lib.fa_last_error().decode() == "FlashAttention only supports fp16 and bf16 data type"


def test_fp8_binders_are_registered():
    import flash_attn_2_cuda as ext
    from flash_attn_amd import backend
    for m in (ext, backend):
        assert callable(m.fwd_fp8) and callable(m.varlen_fwd_fp8)
    q = torch.zeros(1, 4, 2, 64, dtype=FP8)
    for m in (ext, backend):
        with pytest.raises(RuntimeError, match="CUDA"):
            m.fwd_fp8(q, q, q, None, None, None, None, 0.125, False, -1, -1)


def test_fp8_custom_ops_and_fakes():
    from flash_attn_amd import flash_attn_interface as fi
    ns = torch.ops.flash_attn_amd
    assert hasattr(ns, "_flash_attn_fp8_forward") and hasattr(ns, "_flash_attn_varlen_fp8_forward")
    with FakeTensorMode():
        q = torch.empty(2, 100, 4, 128, device="cuda", dtype=FP8)
        k = torch.empty(2, 130, 2, 128, device="cuda", dtype=FP8)
        ds = torch.empty(2, 2, device="cuda", dtype=torch.float32)
        out, lse = fi._flash_attn_fp8_forward(q, k, k, ds, ds, ds, 0.125, True, -1, -1)
        assert out.shape == q.shape and out.dtype == torch.bfloat16
        assert lse.shape == (2, 4, 100) and lse.dtype == torch.float32
        qv = torch.empty(230, 4, 64, device="cuda", dtype=FP8)
        kv = torch.empty(300, 2, 64, device="cuda", dtype=FP8)
        cu = torch.empty(4, device="cuda", dtype=torch.int32)
        out, lse = fi._flash_attn_varlen_fp8_forward(qv, kv, kv, cu, cu, 100, 120, None, None, None, 0.125, False, -1, -1)
        assert out.shape == qv.shape and out.dtype == torch.bfloat16 and lse.shape == (4, 230) and lse.dtype == torch.float32
        # the public functions route fp8 inputs to those ops; return_attn_probs gives (out, lse, None)
        out, lse, p = fi.flash_attn_func(q, k, k, causal=True, return_attn_probs=True, q_descale=ds, k_descale=ds, v_descale=ds)
        assert out.dtype == torch.bfloat16 and out.shape == q.shape and lse.shape == (2, 4, 100) and p is None
        out = fi.flash_attn_varlen_func(qv, kv, kv, cu, cu, 100, 120, k_descale=torch.empty(3, 2, device="cuda"))
        assert out.dtype == torch.bfloat16 and out.shape == qv.shape


def test_fp8_wrapper_checks_run_under_fake_tensors():
    from flash_attn_amd import flash_attn_interface as fi
    with FakeTensorMode():
        q = torch.empty(2, 64, 4, 64, device="cuda", dtype=FP8)
        k = torch.empty(2, 64, 2, 64, device="cuda", dtype=FP8)
        with pytest.raises(RuntimeError, match="k_descale must have shape"):
            fi.flash_attn_func(q, k, k, k_descale=torch.empty(2, 4, device="cuda"))
        with pytest.raises(RuntimeError, match="v_descale must have shape"):
            fi.flash_attn_func(q, k, k, v_descale=torch.empty(4, device="cuda"))
        qb = torch.empty(2, 64, 4, 64, device="cuda", dtype=torch.bfloat16)
        with pytest.raises(RuntimeError, match="float8_e4m3fn inputs only"):
            fi.flash_attn_func(qb, qb, qb, q_descale=torch.empty(2, 4, device="cuda"))
        with pytest.raises(RuntimeError, match="no backward"):
            fi.flash_attn_func(q.requires_grad_(), k, k)
        with torch.no_grad():
            assert fi.flash_attn_func(q, k, k).dtype == torch.bfloat16
        with pytest.raises(RuntimeError, match="dropout"):
            fi.flash_attn_func(k, k, k, dropout_p=0.1)


def test_hazard_check_prices_the_scaled_fp8_mfma():
    spec = importlib.util.spec_from_file_location("isa_mfma_hazards", os.path.join(ROOT, "tools", "isa_mfma_hazards.py"))
    haz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(haz)
    assert haz.passes_of("v_mfma_scale_f32_32x32x64_f8f6f4") == 16
    assert haz.passes_of("v_mfma_scale_f32_16x16x128_f8f6f4") == 8
    assert haz.passes_of("v_mfma_scale_f32_32x32x64_f8f6f4", "v[0:15], v[16:19], v[20:23], v[0:15], v1, v2 cbsz:4 blgp:4") == 8
    assert haz.passes_of("v_mfma_f32_32x32x16_fp8_fp8") == 8 and haz.passes_of("v_mfma_f32_32x32x16_bf16") == 8
    mf = "\tv_mfma_scale_f32_32x32x64_f8f6f4 v[0:15], v[16:23], v[24:31], v[0:15], v32, v32\n"
    pad = "\tv_add_f32 v40, v41, v42\n"
    assert [(h[1], h[2]) for h in haz.scan("_Zk:\n" + mf + pad * 11 + "\tv_max3_f32 v4, v0, v1, v2\n")] == [(11, 19)]
    assert haz.scan("_Zk:\n" + mf + pad * 19 + "\tv_max3_f32 v4, v0, v1, v2\n") == []
