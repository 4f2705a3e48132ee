"""Learnable attention sinks as an exact post-pass (libfa_gfx950_sink.so, include/fa_gfx950_sink.h).

A sink is one learnable logit per QUERY head that joins the softmax denominator and carries no value row (gpt-oss style models; the reference's
``learnable_sink``).  It factors out of the attention kernels: with ``(out, lse)`` what any attention function of this package returns and ``s`` the
sink of a row's head,

    lse' = log(exp(lse) + exp(s)),     out' = sigmoid(lse - s) * out

    out, lse = apply_attn_sink(out, lse, learnable_sink)                                # (B, S, H, D) / (B, H, S), or (total, H, D) / (H, total)
    apply_attn_sink(out, lse, learnable_sink, out_=out, lse_=lse)                       # in place: one read and one write of out
    out = flash_attn_sink_func(q, k, v, learnable_sink, causal=True, window_size=(127, 0))      # training: dq, dk, dv and dsink
    out = flash_attn_varlen_sink_func(q, k, v, learnable_sink, cu_q, cu_k, max_q, max_k, causal=True)
    out = flash_attn_with_kvcache_sink(q, k_cache, v_cache, learnable_sink, cache_seqlens=lens)   # decode: every flash_attn_with_kvcache argument

One kernel launch, fp32 arithmetic, one rounding of out' to its dtype.  A row whose lse is +inf (what this package returns for a row without a visible
key) or -inf has out' = 0, lse' = s, and its ``out`` row is not read.  A sink of -inf is the identity, bit for bit.  The sink is not soft-capped.

Training.  The unchanged backward kernels, handed ``(out', lse')``, recompute the sinked probabilities and return ``softmax_d = rowsum(dout * out')``;
the sink's gradient is ``dsink[h] = -sum_rows exp(s_h - lse') * softmax_d`` (a second small kernel, bit-reproducible: no atomics).  Dropout is refused:
what ``softmax_d`` holds under dropout is the kernels' own business.

Partial results.  MERGE FIRST, APPLY THE SINK ONCE: a chunked-context or prefix / suffix result goes through ``merge_attn_states`` and the sink is
applied to the merged ``(out, lse)``.  Applying the sink to each partial and merging afterwards counts exp(s) once per partial and is wrong.

``apply_attn_sink`` itself has no autograd formula (the attention ops ignore a gradient that arrives at their lse output, so a formula here would
silently drop a term): under grad mode it refuses tensors that require grad; use the ``*_sink_func`` functions.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _cabi_sink as _c
from .flash_attn_interface import (_check_head_dims, _flash_attn_backward, _flash_attn_forward, _flash_attn_varlen_backward,
                                   _flash_attn_varlen_forward, _pad_head_dim, flash_attn_with_kvcache)

_O_DTYPES = {torch.float16: _c.FA_SINK_DTYPE_FP16, torch.bfloat16: _c.FA_SINK_DTYPE_BF16}
_SINK_DTYPES = {torch.float16: _c.FA_SINK_DTYPE_FP16, torch.bfloat16: _c.FA_SINK_DTYPE_BF16, torch.float32: _c.FA_SINK_DTYPE_FP32}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _o_strides(t: torch.Tensor):
    """(batch, row, head) strides of an out tensor: (B, S, H, D) or (total, H, D) = the B = 1 case."""
    return (t.stride(0), t.stride(1), t.stride(2)) if t.dim() == 4 else (0, t.stride(0), t.stride(1))


def _l_strides(t: torch.Tensor):
    """(batch, row, head) strides of an lse-shaped tensor: (B, H, S) or (H, total)."""
    return (t.stride(0), t.stride(2), t.stride(1)) if t.dim() == 3 else (0, t.stride(1), t.stride(0))


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


# ---- the raw ops (namespace flash_attn_amd), with fake implementations: torch.compile / export trace through them without graph breaks -----------------
def _launch_apply(out, lse, sink, o_dst, l_dst, l_bwd) -> None:
    a = _c.FaSinkApplyParams()
    a.out_in, a.lse_in, a.sink, a.out, a.lse, a.lse_bwd = _ptr(out), _ptr(lse), _ptr(sink), _ptr(o_dst), _ptr(l_dst), _ptr(l_bwd)
    a.out_in_batch_stride, a.out_in_row_stride, a.out_in_head_stride = _o_strides(out)
    a.out_batch_stride, a.out_row_stride, a.out_head_stride = _o_strides(o_dst)
    a.lse_in_batch_stride, a.lse_in_row_stride, a.lse_in_head_stride = _l_strides(lse)
    a.lse_batch_stride, a.lse_row_stride, a.lse_head_stride = _l_strides(l_dst)
    if l_bwd is not None:
        a.lse_bwd_batch_stride, a.lse_bwd_row_stride, a.lse_bwd_head_stride = _l_strides(l_bwd)
    a.sink_stride, a.dtype, a.sink_dtype = sink.stride(0), _O_DTYPES[out.dtype], _SINK_DTYPES[sink.dtype]
    if out.dim() == 4:
        a.b, a.s, a.h, a.d = out.shape
    else:
        a.b, (a.s, a.h, a.d) = 1, out.shape
    lib = _c.load()
    with torch.cuda.device(out.device):
        _c.check(lib.fa_sink_apply(C.byref(a), _stream(out)))


def _apply_impl(out: torch.Tensor, lse: torch.Tensor, sink: torch.Tensor, out_: Optional[torch.Tensor], lse_: Optional[torch.Tensor],
                want_lse_bwd: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Out of place: `out` and `lse` are only read.  -> (out', lse', lse_bwd): each a fresh tensor, or an empty one where the result was written to a
    destination (`out_` / `lse_`) or not asked for."""
    o_dst = out_ if out_ is not None else torch.empty(out.shape, dtype=out.dtype, device=out.device)
    l_dst = lse_ if lse_ is not None else torch.empty(lse.shape, dtype=torch.float32, device=out.device)
    l_bwd = torch.empty(lse.shape, dtype=torch.float32, device=out.device) if want_lse_bwd else None
    _launch_apply(out, lse, sink, o_dst, l_dst, l_bwd)
    return (o_dst if out_ is None else out.new_empty((0,)), l_dst if lse_ is None else lse.new_empty((0,)), l_bwd if want_lse_bwd else lse.new_empty((0,)))


def _apply_fake(out, lse, sink, out_, lse_, want_lse_bwd):
    dev = out.device
    return (torch.empty(out.shape if out_ is None else (0,), dtype=out.dtype, device=dev),
            torch.empty(lse.shape if lse_ is None else (0,), dtype=torch.float32, device=dev),
            torch.empty(lse.shape if want_lse_bwd else (0,), dtype=torch.float32, device=dev))


def _apply_inplace_impl(out: torch.Tensor, lse: torch.Tensor, sink: torch.Tensor, want_lse_bwd: bool) -> torch.Tensor:
    """In place: out <- out', lse <- lse' (one read and one write of out).  -> lse_bwd, or an empty tensor where it was not asked for."""
    l_bwd = torch.empty(lse.shape, dtype=torch.float32, device=out.device) if want_lse_bwd else None
    _launch_apply(out, lse, sink, out, lse, l_bwd)
    return l_bwd if want_lse_bwd else lse.new_empty((0,))


def _apply_inplace_fake(out, lse, sink, want_lse_bwd):
    return torch.empty(lse.shape if want_lse_bwd else (0,), dtype=torch.float32, device=out.device)


def _apply_out_inplace_impl(out: torch.Tensor, lse: torch.Tensor, sink: torch.Tensor, lse_: torch.Tensor) -> None:
    """out <- out' in place, lse' written to `lse_` (another tensor than `lse`, which is only read)."""
    _launch_apply(out, lse, sink, out, lse_, None)


def _apply_out_inplace_fake(out, lse, sink, lse_):
    return None


def _dsink_impl(softmax_d: torch.Tensor, lse_bwd: torch.Tensor, sink: torch.Tensor) -> torch.Tensor:
    """softmax_d, lse_bwd: fp32 (B, H, S) or (H, total), any strides -> dsink fp32 (H)."""
    if softmax_d.dim() not in (2, 3) or softmax_d.shape != lse_bwd.shape or softmax_d.dtype != torch.float32 or lse_bwd.dtype != torch.float32:
        raise RuntimeError(f"_attn_sink_dsink: softmax_d and lse_bwd must be fp32 tensors of one shape, (batch, heads, seqlen) or (heads, total): got "
                           f"{tuple(softmax_d.shape)} {softmax_d.dtype} and {tuple(lse_bwd.shape)} {lse_bwd.dtype}")
    h = softmax_d.shape[-2]
    if tuple(sink.shape) != (h,) or sink.dtype not in _SINK_DTYPES:
        raise RuntimeError(f"_attn_sink_dsink: learnable_sink must be fp32 / bf16 / fp16 of shape ({h},), got {tuple(sink.shape)} {sink.dtype}")
    dsink = torch.empty((h,), dtype=torch.float32, device=softmax_d.device)
    a = _c.FaSinkDsinkParams()
    a.softmax_d_batch_stride, a.softmax_d_row_stride, a.softmax_d_head_stride = _l_strides(softmax_d)
    a.lse_bwd_batch_stride, a.lse_bwd_row_stride, a.lse_bwd_head_stride = _l_strides(lse_bwd)
    a.sink_stride, a.dsink_stride, a.sink_dtype = sink.stride(0), 1, _SINK_DTYPES[sink.dtype]
    a.b, a.s, a.h = (softmax_d.shape[0], softmax_d.shape[2], h) if softmax_d.dim() == 3 else (1, softmax_d.shape[1], h)
    lib = _c.load()
    need = int(lib.fa_sink_dsink_workspace_bytes(C.byref(a)))
    ws = torch.empty((max(need, 4) // 4,), dtype=torch.float32, device=softmax_d.device)   # (the caching allocator: no host synchronisation)
    a.softmax_d, a.lse_bwd, a.sink, a.dsink, a.workspace, a.workspace_bytes = _ptr(softmax_d), _ptr(lse_bwd), _ptr(sink), _ptr(dsink), _ptr(ws), ws.numel() * 4
    with torch.cuda.device(softmax_d.device):
        _c.check(lib.fa_sink_dsink(C.byref(a), _stream(softmax_d)))
    return dsink


def _dsink_fake(softmax_d, lse_bwd, sink):
    return torch.empty((softmax_d.shape[-2],), dtype=torch.float32, device=softmax_d.device)


def _register(name, impl, fake, mutates=()):
    op = torch.library.custom_op(f"flash_attn_amd::{name}", impl, mutates_args=mutates, device_types="cuda")
    op.register_fake(fake)
    return getattr(torch.ops.flash_attn_amd, name)


# (three ops, so that each declares as mutated only what it writes: the out-of-place call leaves the version counters of `out` / `lse` alone and costs
# torch.compile no copy back.  Passing ONE tensor twice, as input and as destination, would alias a mutated argument, which functionalisation cannot express
# -- hence an op of its own for the in-place call)
_attn_sink_apply = _register("_attn_sink_apply", _apply_impl, _apply_fake, ("out_", "lse_"))
_attn_sink_apply_ = _register("_attn_sink_apply_", _apply_inplace_impl, _apply_inplace_fake, ("out", "lse"))
_attn_sink_apply_out_ = _register("_attn_sink_apply_out_", _apply_out_inplace_impl, _apply_out_inplace_fake, ("out", "lse_"))
_attn_sink_dsink = _register("_attn_sink_dsink", _dsink_impl, _dsink_fake)


# ---- checks: shapes, dtypes and devices only, before the library is needed ----------------------------------------------------------------------------
def _check_sink(fn: str, sink, nheads: int, device) -> None:
    if not isinstance(sink, torch.Tensor):
        raise RuntimeError(f"{fn}: learnable_sink must be a tensor of shape (nheads_q,) = ({nheads},)")
    if tuple(sink.shape) != (nheads,):
        raise RuntimeError(f"{fn}: learnable_sink must have shape (nheads_q,) = ({nheads},), got {tuple(sink.shape)}")
    if sink.dtype not in _SINK_DTYPES:
        raise RuntimeError(f"{fn}: learnable_sink must be fp32, bf16 or fp16 (got {sink.dtype})")
    if sink.device != device:
        raise RuntimeError(f"{fn}: learnable_sink must be on the device of the other tensors ({device}), got {sink.device}")


def _is(a: Optional[torch.Tensor], b: torch.Tensor) -> bool:
    """a is the tensor b, or a view of the same elements (no data pointers: this runs under fake tensors as well)."""
    return a is not None and (a is b or (torch._C._is_alias_of(a, b) and a.storage_offset() == b.storage_offset() and a.shape == b.shape
                                         and a.stride() == b.stride() and a.dtype == b.dtype))


def apply_attn_sink(out: torch.Tensor, lse: torch.Tensor, learnable_sink: torch.Tensor, *, out_: Optional[torch.Tensor] = None,
                    lse_: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Join a learnable sink to a finished attention result: lse' = log(exp(lse) + exp(s)), out' = sigmoid(lse - s) * out.

    out: (B, S, H, D) with lse (B, H, S), or (total, H, D) with (H, total): what flash_attn_func(..., return_attn_probs=True), flash_attn_varlen_func,
    flash_attn_with_kvcache(..., return_softmax_lse=True) and merge_attn_states return, or views of those with a contiguous last dimension of out,
    16-byte aligned data and out strides that are multiples of 16 bytes; bf16 or fp16, D % 8 == 0, D <= 512; lse fp32, any strides.
    learnable_sink: (H,) fp32 / bf16 / fp16.  A row whose lse is +inf or -inf (no visible key) gets out' = 0 and lse' = s, and its out row is not
    read; a sink of -inf changes nothing, bit for bit.  For a result in parts: merge the parts first, then apply the sink ONCE.

    `out_` / `lse_`: written in place; otherwise new contiguous tensors.  `out_=out, lse_=lse` is the in-place call (one pass over out); any other
    overlap between an input and an output is refused.  Returns (out', lse').  No backward: see flash_attn_sink_func."""
    fn = "apply_attn_sink"
    if torch.is_grad_enabled() and any(t is not None and isinstance(t, torch.Tensor) and t.requires_grad for t in (out, lse, learnable_sink, out_, lse_)):
        raise RuntimeError(f"{fn} has no backward: call it under torch.no_grad() or on tensors that do not require grad; "
                           "flash_attn_sink_func / flash_attn_varlen_sink_func are the functions with gradients (dq, dk, dv and dsink)")
    if out.dim() not in (3, 4):
        raise RuntimeError(f"{fn}: out must be (batch, seqlen, heads, head_size) or (total, heads, head_size)")
    lse_shape = tuple(out.shape[:-3]) + (out.shape[-2], out.shape[-3])
    for name, o, l in (("", out, lse), ("_", out_, lse_)):
        if o is not None:
            if tuple(o.shape) != tuple(out.shape) or o.dtype != out.dtype:
                raise RuntimeError(f"{fn}: out{name} must have the shape and dtype of out {tuple(out.shape)} {out.dtype}, got {tuple(o.shape)} {o.dtype}")
            if o.dtype not in _O_DTYPES:
                raise RuntimeError(f"{fn}: out{name} must be bf16 or fp16 (got {o.dtype})")
            if o.stride(-1) != 1:
                raise RuntimeError(f"{fn}: out{name} must have a contiguous last dimension")
        if l is not None:
            if tuple(l.shape) != lse_shape:
                raise RuntimeError(f"{fn}: lse{name} must have shape (.., heads, seqlen) = {lse_shape}, got {tuple(l.shape)}")
            if l.dtype != torch.float32:
                raise RuntimeError(f"{fn}: lse{name} must be fp32 (got {l.dtype})")
    d = out.shape[-1]
    if d % 8 != 0 or d < 8 or d > 512:
        raise RuntimeError(f"{fn}: head_size must be a multiple of 8 in [8, 512] (got {d})")
    _check_sink(fn, learnable_sink, out.shape[-2], out.device)
    for t in (out, lse, out_, lse_):
        if t is not None and (not t.is_cuda or t.device != out.device):
            raise RuntimeError(f"{fn}: every tensor must be on the same CUDA device")
    o_here, l_here = _is(out_, out), _is(lse_, lse)
    if o_here and l_here:
        _attn_sink_apply_(out, lse, learnable_sink, False)
    elif o_here:                                    # out in place, lse' elsewhere
        if lse_ is None:
            lse_ = torch.empty(lse.shape, dtype=torch.float32, device=out.device)
        _attn_sink_apply_out_(out, lse, learnable_sink, lse_)
    elif l_here:                                    # lse in place, out' elsewhere
        o, l, _ = _attn_sink_apply(out, lse, learnable_sink, out_, None, False)
        lse.copy_(l)
        return (o if out_ is None else out_), lse_
    else:
        o, l, _ = _attn_sink_apply(out, lse, learnable_sink, out_, lse_, False)
        return (o if out_ is None else out_), (l if lse_ is None else lse_)
    return out_, lse_


def _refuse(fn: str, q, k, v, dropout_p: float) -> None:
    if dropout_p != 0.0:
        raise RuntimeError(f"{fn}: dropout is not supported with a learnable sink (dsink rests on the backward's softmax_d, which is unspecified under dropout)")
    if any(t.dtype == torch.float8_e4m3fn for t in (q, k, v)):
        raise RuntimeError(f"{fn}: float8_e4m3fn q / k / v are not supported with a learnable sink (the fp8 forward has no backward); "
                           "for inference apply apply_attn_sink to the result of flash_attn_func")


class _SinkAttnFn(torch.autograd.Function):
    """_AttnFn with the sink joined after the forward kernel; the backward kernels run on (out', lse_bwd) and their softmax_d gives dsink."""

    @staticmethod
    def forward(ctx, q, k, v, sink, softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic, is_grad_enabled):
        needs_grad = is_grad_enabled and any(t.requires_grad for t in (q, k, v, sink))
        if softmax_scale is None:
            softmax_scale = q.shape[-1] ** (-0.5)
        d_orig, dv_orig = q.shape[-1], v.shape[-1]
        if not _check_head_dims("flash_attn_sink_func", q, v, 0.0, softcap, alibi_slopes, False):
            q, k, v = _pad_head_dim(q, k, v)
        out_p, lse, _, rng_state = _flash_attn_forward(q, k, v, 0.0, softmax_scale, causal, window_size[0], window_size[1], softcap, alibi_slopes, False)
        lse_bwd = _attn_sink_apply_(out_p, lse, sink, needs_grad)
        if needs_grad:
            ctx.save_for_backward(q, k, v, out_p, lse_bwd, sink, rng_state)
            ctx.cfg = (softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic, d_orig, dv_orig)
        ctx.mark_non_differentiable(lse)
        return out_p[..., :dv_orig], lse

    @staticmethod
    def backward(ctx, dout, *unused):
        q, k, v, out, lse_bwd, sink, rng_state = ctx.saved_tensors
        softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic, d_orig, dv_orig = ctx.cfg
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        (dout_p,) = _pad_head_dim(dout) if dout.shape[-1] % 8 else (dout,)
        softmax_d = _flash_attn_backward(dout_p, q, k, v, out, lse_bwd, dq, dk, dv, 0.0, softmax_scale, causal, window_size[0], window_size[1], softcap,
                                         alibi_slopes, deterministic, rng_state)
        dsink = _attn_sink_dsink(softmax_d, lse_bwd, sink).to(sink.dtype) if ctx.needs_input_grad[3] else None
        return (dq[..., :d_orig], dk[..., :d_orig], dv[..., :dv_orig], dsink) + (None,) * 7


class _VarlenSinkAttnFn(torch.autograd.Function):
    """_VarlenAttnFn with the sink joined after the forward kernel."""

    @staticmethod
    def forward(ctx, q, k, v, sink, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, softmax_scale, causal, window_size, softcap, alibi_slopes,
                deterministic, is_grad_enabled):
        needs_grad = is_grad_enabled and any(t.requires_grad for t in (q, k, v, sink))
        if softmax_scale is None:
            softmax_scale = q.shape[-1] ** (-0.5)
        d_orig, dv_orig = q.shape[-1], v.shape[-1]
        if not _check_head_dims("flash_attn_varlen_sink_func", q, v, 0.0, softcap, alibi_slopes, False, None):
            q, k, v = _pad_head_dim(q, k, v)
        out_p, lse, _, rng_state = _flash_attn_varlen_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, 0.0, softmax_scale, causal,
                                                              window_size[0], window_size[1], softcap, alibi_slopes, False, None)
        lse_bwd = _attn_sink_apply_(out_p, lse, sink, needs_grad)
        if needs_grad:
            ctx.save_for_backward(q, k, v, out_p, lse_bwd, sink, cu_seqlens_q, cu_seqlens_k, rng_state)
            ctx.cfg = (max_seqlen_q, max_seqlen_k, softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic, d_orig, dv_orig)
        ctx.mark_non_differentiable(lse)
        return out_p[..., :dv_orig], lse

    @staticmethod
    def backward(ctx, dout, *unused):
        q, k, v, out, lse_bwd, sink, cu_q, cu_k, rng_state = ctx.saved_tensors
        mq, mk, softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic, d_orig, dv_orig = ctx.cfg
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        (dout_p,) = _pad_head_dim(dout) if dout.shape[-1] % 8 else (dout,)
        softmax_d = _flash_attn_varlen_backward(dout_p, q, k, v, out, lse_bwd, dq, dk, dv, cu_q, cu_k, mq, mk, 0.0, softmax_scale, causal, window_size[0],
                                                window_size[1], softcap, alibi_slopes, deterministic, rng_state)
        dsink = _attn_sink_dsink(softmax_d, lse_bwd, sink).to(sink.dtype) if ctx.needs_input_grad[3] else None
        return (dq[..., :d_orig], dk[..., :d_orig], dv[..., :dv_orig], dsink) + (None,) * 11


def flash_attn_sink_func(q, k, v, learnable_sink, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0, alibi_slopes=None,
                         deterministic=False, return_attn_probs=False, *, dropout_p=0.0):
    """flash_attn_func with a learnable sink per query head: learnable_sink (H,) fp32 / bf16 / fp16 on q's device.

    q (B,Sq,H,D); k, v (B,Sk,Hk,D): everything flash_attn_func takes (MQA / GQA, causal, window, softcap -- the sink is not capped --, ALiBi, every
    head dim, the (192, 128) pair) except dropout and float8_e4m3fn inputs.  Gradients: dq, dk, dv, and dsink in the sink's dtype (skipped when the
    sink does not require grad).  Returns out (B,Sq,H,D); with ``return_attn_probs`` (out, lse', None), lse' = log(exp(lse) + exp(sink)) and the sink
    itself on rows without a visible key (their out is 0)."""
    fn = "flash_attn_sink_func"
    _refuse(fn, q, k, v, dropout_p)
    _check_sink(fn, learnable_sink, q.shape[-2], q.device)
    out, lse = _SinkAttnFn.apply(q, k, v, learnable_sink, softmax_scale, causal, tuple(window_size), softcap, alibi_slopes, deterministic,
                                 torch.is_grad_enabled())
    return (out, lse, None) if return_attn_probs else out


def flash_attn_varlen_sink_func(q, k, v, learnable_sink, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, softmax_scale=None, causal=False,
                                window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False, return_attn_probs=False, *, dropout_p=0.0):
    """flash_attn_varlen_func with a learnable sink per query head: q (total_q,H,D); k, v (total_k,Hk,D); cu_seqlens_* int32 (B+1).  As
    flash_attn_sink_func; with ``return_attn_probs`` (out, lse' (H,total_q), None)."""
    fn = "flash_attn_varlen_sink_func"
    _refuse(fn, q, k, v, dropout_p)
    _check_sink(fn, learnable_sink, q.shape[-2], q.device)
    out, lse = _VarlenSinkAttnFn.apply(q, k, v, learnable_sink, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, softmax_scale, causal,
                                       tuple(window_size), softcap, alibi_slopes, deterministic, torch.is_grad_enabled())
    return (out, lse, None) if return_attn_probs else out


def flash_attn_with_kvcache_sink(q, k_cache, v_cache, learnable_sink, **kwargs):
    """flash_attn_with_kvcache with a learnable sink per query head, joined in place to the kernel's (out, lse): every keyword of
    flash_attn_with_kvcache passes through (append, paged caches, cache_batch_idx, num_splits, the fp8 cache with its descales).  Returns out', or
    (out', lse') with ``return_softmax_lse=True``.  No backward."""
    fn = "flash_attn_with_kvcache_sink"
    _check_sink(fn, learnable_sink, q.shape[-2], q.device)
    want_lse = bool(kwargs.pop("return_softmax_lse", False))
    with torch.no_grad():
        out, lse = flash_attn_with_kvcache(q, k_cache, v_cache, return_softmax_lse=True, **kwargs)
        _attn_sink_apply_(out, lse, learnable_sink, False)
    return (out, lse) if want_lse else out
