"""CPU suite of a v / o head dim that differs from q / k (D = 192, Dv = 128): the custom-op fakes and tracing under fake tensors, the refusals
of the public functions (checked on shapes and flags, before the backend), and the C ABI -- struct sizes, FA_ERR_UNSUPPORTED answers and the
host-side queries, all of which answer without a device (as tests/test_kvcache_fp8_cpu.py does for its path)."""
import ctypes as C
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, DV = 192, 128
BF = torch.bfloat16


def _lib():
    from flash_attn_amd import _cabi
    return _cabi, _cabi.load()


def _qkv(B=2, Sq=100, Sk=130, H=4, Hk=2, d=D, dv=DV, dtype=BF):
    return (torch.empty(B, Sq, H, d, device="cuda", dtype=dtype), torch.empty(B, Sk, Hk, d, device="cuda", dtype=dtype),
            torch.empty(B, Sk, Hk, dv, device="cuda", dtype=dtype))


# ---------------------------------------------------------------- fake tensors
def test_fakes_give_dv_wide_outputs():
    from flash_attn_amd import flash_attn_interface as fi
    with FakeTensorMode():
        q, k, v = _qkv()
        out, lse, p, rng = fi._flash_attn_forward(q, k, v, 0.0, D ** -0.5, True, -1, -1, 0.0, None, False)
        assert out.shape == (2, 100, 4, DV) and lse.shape == (2, 4, 100) and lse.dtype == torch.float32
        out, lse, _ = fi.flash_attn_func(q, k, v, causal=True, return_attn_probs=True)
        assert out.shape[-1] == DV and out.shape == (2, 100, 4, DV) and lse.shape == (2, 4, 100)
        qv = torch.empty(230, 4, D, device="cuda", dtype=torch.float16)
        kv = torch.empty(300, 2, D, device="cuda", dtype=torch.float16)
        vv = torch.empty(300, 2, DV, device="cuda", dtype=torch.float16)
        cu = torch.empty(4, device="cuda", dtype=torch.int32)
        out, lse, p, rng = fi._flash_attn_varlen_forward(qv, kv, vv, cu, cu, 100, 120, 0.0, D ** -0.5, False)
        assert out.shape == (230, 4, DV) and lse.shape == (4, 230)
        out, lse, _ = fi.flash_attn_varlen_func(qv, kv, vv, cu, cu, 100, 120, causal=True, return_attn_probs=True)
        assert out.shape == (230, 4, DV) and lse.shape == (4, 230)
        # Dv = D keeps q's shape (and, as before, its layout)
        out = fi.flash_attn_func(q, k, k)
        assert out.shape == q.shape


def test_export_traces_the_public_function():
    from flash_attn_amd import flash_attn_interface as fi

    class M(torch.nn.Module):
        def forward(self, q, k, v):
            return fi.flash_attn_func(q, k, v, causal=True)

    with FakeTensorMode():
        q, k, v = _qkv()
    ep = torch.export.export(M(), (q, k, v))
    assert any("flash_attn_amd" in str(n.target) for n in ep.graph.nodes), "the custom op must appear in the exported graph"
    outs = [n for n in ep.graph.nodes if n.op == "output"]
    val = outs[0].args[0][0].meta["val"]
    assert tuple(val.shape) == (2, 100, 4, DV)


# ---------------------------------------------------------------- refusals of the public functions
def test_public_refusals_name_the_head_dims_or_the_argument():
    from flash_attn_amd import flash_attn_interface as fi
    with FakeTensorMode():
        q, k, v = _qkv()
        cases = [
            (lambda: fi.flash_attn_func(q, k, v[..., :96]), r"192.*96"),                                   # any other pair
            (lambda: fi.flash_attn_func(q[..., :128], k[..., :128], v[..., :96]), r"128.*96"),
            (lambda: fi.flash_attn_func(q, k, torch.empty(2, 130, 2, 256, device="cuda", dtype=BF)), r"192.*256"),
            (lambda: fi.flash_attn_func(q, k, v, dropout_p=0.1), r"192.*128.*dropout"),
            (lambda: fi.flash_attn_func(q, k, v, softcap=30.0), r"192.*128.*softcap"),
            (lambda: fi.flash_attn_func(q, k, v, alibi_slopes=torch.empty(4, device="cuda")), r"192.*128.*alibi_slopes"),
            (lambda: fi.flash_attn_padded_func(q, k, v, torch.empty(2, device="cuda", dtype=torch.int32),
                                               torch.empty(2, device="cuda", dtype=torch.int32)), r"flash_attn_padded_func.*192.*128"),
            (lambda: fi.flash_attn_with_kvcache(q, k, v), r"flash_attn_with_kvcache.*192.*128"),
        ]
        qv = torch.empty(230, 4, D, device="cuda", dtype=BF)
        kv = torch.empty(4, 256, 2, D, device="cuda", dtype=BF)
        vv = torch.empty(4, 256, 2, DV, device="cuda", dtype=BF)
        cu = torch.empty(3, device="cuda", dtype=torch.int32)
        bt = torch.empty(2, 2, device="cuda", dtype=torch.int32)
        cases.append((lambda: fi.flash_attn_varlen_func(qv, kv, vv, cu, cu, 100, 100, block_table=bt), r"192.*128.*block_table"))
        f8 = torch.float8_e4m3fn
        cases.append((lambda: fi.flash_attn_func(q.to(f8), k.to(f8), v.to(f8)), r"fp8.*192.*128"))
        for fn, pat in cases:
            with pytest.raises(RuntimeError, match=pat):
                fn()


def test_return_softmax_and_leftpad_are_refused_by_the_binder_checks():
    from flash_attn_amd import backend as be
    for kw, pat in ((dict(return_softmax=True), r"192.*128.*return_softmax"), (dict(leftpad_k=object()), r"192.*128.*leftpad_k"),
                    (dict(block_table=object()), r"192.*128.*block_table"), (dict(p_dropout=0.5), r"192.*128.*p_dropout")):
        with pytest.raises(RuntimeError, match=pat):
            be.check_head_dim_pair("varlen_fwd", D, DV, **kw)
    be.check_head_dim_pair("fwd", D, DV)
    be.check_head_dim_pair("fwd", 128, 128, p_dropout=0.5, softcap=1.0)   # Dv = D: nothing to refuse here, the old route decides
    assert be.FWD_KERNEL_NAMES[6] == "fa_fwd_dv_kernel" and be._SCHED_FIELDS[-1] == "dv" and len(be._SCHED_FIELDS) == 13


# ---------------------------------------------------------------- C ABI
def _fwd_params(_cabi, **kw):
    a = _cabi.FaFwdParams()
    for n in ("q", "k", "v", "o", "softmax_lse"):
        setattr(a, n, C.c_void_p(4096))   # never dereferenced: every case below is answered before a launch
    a.b, a.h, a.h_k, a.d, a.d_v, a.seqlen_q, a.seqlen_k, a.total_q = 2, 4, 2, D, DV, 256, 256, 512
    a.dtype, a.softmax_scale, a.window_left, a.window_right = _cabi.FA_DTYPE_BF16, D ** -0.5, -1, -1
    for n, x in kw.items():
        setattr(a, n, x)
    return a


def _bwd_params(_cabi, **kw):
    a = _cabi.FaBwdParams()
    a.b, a.h, a.h_k, a.d, a.d_v, a.seqlen_q, a.seqlen_k, a.total_q, a.total_k = 2, 4, 2, D, DV, 256, 256, 512, 512
    a.dtype, a.softmax_scale, a.window_left, a.window_right = _cabi.FA_DTYPE_BF16, D ** -0.5, -1, -1
    for n, x in kw.items():
        setattr(a, n, x)
    return a


def test_struct_sizes_and_abi_version_are_those_of_the_parent_commit():
    _cabi, lib = _lib()
    # read on the parent commit: d_v took reserved slots, nothing moved
    assert lib.fa_sizeof_fwd_params() == C.sizeof(_cabi.FaFwdParams) == 344
    assert lib.fa_sizeof_bwd_params() == C.sizeof(_cabi.FaBwdParams) == 424
    assert lib.fa_abi_version() == _cabi.FA_ABI_VERSION == 6
    assert _cabi.FaFwdParams.d_v.offset == _cabi.FaFwdParams.p_dropout.offset + 4 and _cabi.FaFwdParams.d_v.size == 4
    assert _cabi.FaBwdParams.d_v.offset == _cabi.FaBwdParams.p_dropout.offset + 4 and _cabi.FaBwdParams.reserved.size == 8
    header = open(os.path.join(ROOT, "include", "fa_gfx950.h")).read()
    assert re.search(r"#define FA_SCHEDULE_FIELDS 13\b", header) and re.search(r"#define FA_ABI_VERSION 6\b", header)
    buf = (C.c_int32 * 16)()
    assert lib.fa_last_schedule(buf, 16) == 13


def test_unsupported_pairs_and_features_answer_before_any_launch():
    _cabi, lib = _lib()
    ptr = C.c_void_p(4096)
    fwd_cases = [
        (lib.fa_fwd, dict(d_v=96), r"192, 96"), (lib.fa_fwd, dict(d=128, d_v=96), r"128, 96"), (lib.fa_fwd, dict(d=64, d_v=256), r"64, 256"),
        (lib.fa_fwd, dict(d=192, d_v=64), r"192, 64"),
        (lib.fa_fwd, dict(p_dropout=0.1, rng_state=ptr), r"192, 128.*dropout"), (lib.fa_fwd, dict(softcap=30.0), r"192, 128.*softcap"),
        (lib.fa_fwd, dict(alibi_slopes=ptr), r"192, 128.*ALiBi"), (lib.fa_fwd, dict(p_dropout=0.0, randval=ptr), r"192, 128.*return_softmax"),
        (lib.fa_varlen_fwd, dict(cu_seqlens_q=ptr, cu_seqlens_k=ptr, block_table=ptr, page_block_size=256), r"192, 128.*block_table"),
        (lib.fa_varlen_fwd, dict(cu_seqlens_q=ptr, cu_seqlens_k=ptr, leftpad_k=ptr), r"192, 128.*leftpad_k"),
        (lib.fa_fwd_kvcache, dict(), r"fa_fwd_kvcache.*192, 128"),
        (lib.fa_fwd_kvcache, dict(seqused_k=ptr, cache_batch_idx=ptr), r"192, 128.*KV-cache"),
    ]
    for fn, kw, pat in fwd_cases:
        rc = fn(C.byref(_fwd_params(_cabi, **kw)), None)
        msg = lib.fa_last_error().decode()
        assert rc == _cabi.FA_ERR_UNSUPPORTED and re.search(pat, msg), (kw, rc, msg)
    for fn in (lib.fa_fwd_fp8, lib.fa_varlen_fwd_fp8, lib.fa_fwd_kvcache_fp8):
        rc = fn(C.byref(_fwd_params(_cabi, dtype=_cabi.FA_DTYPE_FP8_E4M3, d=128, d_v=64)), None, None)
        msg = lib.fa_last_error().decode()
        assert rc == _cabi.FA_ERR_UNSUPPORTED and re.search(r"128, 64.*fp8", msg), (rc, msg)
    for fn, kw, pat in ((lib.fa_bwd, dict(d_v=96), r"192, 96"), (lib.fa_bwd, dict(softcap=30.0), r"192, 128.*softcap"),
                        (lib.fa_bwd, dict(alibi_slopes=ptr), r"192, 128.*ALiBi"), (lib.fa_bwd, dict(p_dropout=0.1, rng_state=ptr), r"192, 128.*dropout"),
                        (lib.fa_varlen_bwd, dict(d=256, d_v=128), r"256, 128")):
        rc = fn(C.byref(_bwd_params(_cabi, **kw)), None)
        msg = lib.fa_last_error().decode()
        assert rc == _cabi.FA_ERR_UNSUPPORTED and re.search(pat, msg), (kw, rc, msg)
    # the built pair passes these checks (and stops at the first pointer check: nothing here has buffers); d_v = 0 and d_v = d mean "as d"
    a = _fwd_params(_cabi, q=None)
    assert lib.fa_fwd(C.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and "non-NULL" in lib.fa_last_error().decode()
    for dv in (0, 128):
        a = _fwd_params(_cabi, d=128, d_v=dv, softcap=30.0, q=None)
        assert lib.fa_fwd(C.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and "non-NULL" in lib.fa_last_error().decode()
    assert lib.fa_fwd(C.byref(_fwd_params(_cabi, d_v=-8)), None) == _cabi.FA_ERR_INVALID_ARGUMENT


def test_schedule_queries_for_the_pair():
    _cabi, lib = _lib()
    assert lib.fa_fwd_schedule_query(C.byref(_fwd_params(_cabi)), 0) == 4
    assert lib.fa_fwd_schedule_query(C.byref(_fwd_params(_cabi, seqlen_q=4096, seqlen_k=4096, b=2, h=32, h_k=32)), 0) == 4
    assert lib.fa_fwd_schedule_query(C.byref(_fwd_params(_cabi, d_v=96)), 0) == _cabi.FA_ERR_UNSUPPORTED
    assert lib.fa_fwd_schedule_query(C.byref(_fwd_params(_cabi, d=128, d_v=0, seqlen_q=4096, seqlen_k=4096, h=32, h_k=32)), 0) == 64   # old route untouched
    for kw in (dict(), dict(seqlen_q=4096, seqlen_k=4096, h=32, h_k=32), dict(seqlen_q=4096, seqlen_k=4096, is_causal=1)):
        assert lib.fa_bwd_dq_schedule_query(C.byref(_bwd_params(_cabi, **kw))) == 4
    assert lib.fa_bwd_dq_schedule_query(C.byref(_bwd_params(_cabi, d_v=96))) == _cabi.FA_ERR_UNSUPPORTED
    # never the fused modes 3 / 5 for this shape
    plan = (C.c_int32 * 8)()
    for kw in (dict(seqlen_q=1024, seqlen_k=1024, h=32, h_k=32, b=8, is_causal=1), dict()):
        assert lib.fa_bwd_plan_query(C.byref(_bwd_params(_cabi, **kw)), plan, 8) == 8 and plan[0] == 0, list(plan)


def test_workspaces_answer_consistently():
    _cabi, lib = _lib()
    al = lambda n: (n + 255) & ~255
    # GQA group split (B2 S1024 H32/2 causal -> 8 virtual heads per group): dK partials at width 192, dV partials at width 128
    a = _bwd_params(_cabi, b=2, h=32, h_k=2, seqlen_q=1024, seqlen_k=1024, total_q=2048, total_k=2048, is_causal=1)
    plan = (C.c_int32 * 8)()
    assert lib.fa_bwd_plan_query(C.byref(a), plan, 8) == 8 and plan[0] == 0
    gs = plan[3]
    assert gs == 8
    assert lib.fa_bwd_workspace_bytes(C.byref(a)) == al(2 * 1024 * 2 * gs * D * 2) + al(2 * 1024 * 2 * gs * DV * 2)
    a.d_v = 0   # D = Dv = 192: both halves at 192, as before
    assert lib.fa_bwd_workspace_bytes(C.byref(a)) == 2 * al(2 * 1024 * 2 * gs * D * 2)
    # forward: fixed-length needs nothing; an uneven packed batch gets the work list of 128-row blocks
    assert lib.fa_fwd_workspace_bytes(C.byref(_fwd_params(_cabi))) == 0
    ptr = C.c_void_p(4096)
    v = _fwd_params(_cabi, cu_seqlens_q=ptr, cu_seqlens_k=ptr, b=5, h=6, h_k=2, seqlen_q=1024, seqlen_k=1024, total_q=1454)
    assert lib.fa_fwd_workspace_bytes(C.byref(v)) == (1454 // 128 + 5 + 1) * 8
