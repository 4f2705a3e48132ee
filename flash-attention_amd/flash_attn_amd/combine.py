"""The merge of partial attention results (libfa_gfx950_combine.so, include/fa_gfx950_combine.h).

Every attention function of this package returns ``(out, lse)``.  Two such results over DISJOINT key sets -- the chunks of a chunked-context (MLA)
prefill, a shared prefix and a per-request suffix, the steps of a ring -- merge exactly:

    lse = log(exp(lse_a) + exp(lse_b)),   out = exp(lse_a - lse) * out_a + exp(lse_b - lse) * out_b

    out, lse = merge_attn_states(out_a, lse_a, out_b, lse_b)                 # this package's layouts: (B, S, H, D) / (B, H, S), (total, H, D) / (H, total)
    merge_attn_states(acc, acc_lse, out_c, lse_c, out=acc, lse=acc_lse)      # the running merge, in place (an fp32 accumulator keeps one rounding at the end)
    out, lse = flash_attn_combine(out_partial, lse_partial)                  # FA3's contract: a stack of splits, (S, B, L, H, D) / (S, B, L, H)

One kernel launch, fp32 arithmetic, one rounding to the output dtype.  A partial whose lse is +inf (what this package returns for a row without a
visible key) or -inf (FA3's marker) is EMPTY: its weight is 0 and its ``out`` row is not read, so NaN or garbage there never reaches the result.  A
row with no live partial gives ``out = 0`` and ``lse = +inf`` (merge_attn_states) or ``-inf`` (flash_attn_combine).  The checks read shapes, dtypes,
devices and strides only; nothing synchronises with the host, so both calls can be captured in a HIP graph.

Training.  Neither function has an autograd formula, and on purpose: the attention ops ignore a gradient that arrives at their lse output, so a
formula here would silently drop the term that flows through the lse.  The exact recipe needs none.  With ``out`` / ``lse`` the MERGED result over
all chunks and ``dout`` its gradient, call, per key chunk c,

    _flash_attn_backward(dout, q, k_c, v_c, out, lse, dq_c, dk_c, dv_c, ...)       # (flash_attn_amd.flash_attn_interface; the varlen twin likewise)

with the mask of that chunk, and sum the ``dq_c``; ``dk_c`` / ``dv_c`` are the chunk's own gradients.  Every chunk's P is recomputed against the
global lse, and delta = rowsum(dout * out) is the global one: that is the monolithic backward, split by key columns.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _cabi_combine as _c

_DTYPES = {torch.float16: _c.FA_COMBINE_DTYPE_FP16, torch.bfloat16: _c.FA_COMBINE_DTYPE_BF16, torch.float32: _c.FA_COMBINE_DTYPE_FP32}
_PATH = _c.FA_COMBINE_PATH_AUTO   # (tests set it to run one kernel on another kernel's shapes)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _refuse_grad(fn: str, *ts) -> None:
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError(f"{fn} has no backward: call it under torch.no_grad() or on tensors that do not require grad "
                           "(the module docstring has the exact training recipe)")


def _same_device(fn: str, *ts) -> None:
    first = ts[0]
    for t in ts:
        if t is not None and (not t.is_cuda or t.device != first.device):
            raise RuntimeError(f"{fn}: every tensor must be on the same CUDA device")


def _launch(sources, out: torch.Tensor, lse: Optional[torch.Tensor], b: int, s: int, h: int, d: int, out_strides, lse_strides, sign: int) -> None:
    """sources: (o, lse, n_splits, (o split / batch / row / head strides), (lse split / batch / row / head strides))."""
    a = _c.FaCombineParams()
    a.n_sources = len(sources)
    for i, (o, l, n, ost, lst) in enumerate(sources):
        sr = a.src[i]
        sr.o, sr.lse, sr.n_splits, sr.dtype = _ptr(o), _ptr(l), n, _DTYPES[o.dtype]
        sr.o_split_stride, sr.o_batch_stride, sr.o_row_stride, sr.o_head_stride = ost
        sr.lse_split_stride, sr.lse_batch_stride, sr.lse_row_stride, sr.lse_head_stride = lst
    a.out, a.lse, a.out_dtype = _ptr(out), _ptr(lse), _DTYPES[out.dtype]
    a.out_batch_stride, a.out_row_stride, a.out_head_stride = out_strides
    if lse is not None:
        a.lse_batch_stride, a.lse_row_stride, a.lse_head_stride = lse_strides
    a.b, a.s, a.h, a.d, a.empty_lse_sign, a.path = b, s, h, d, sign, _PATH
    lib = _c.load()
    with torch.cuda.device(out.device):
        _c.check(lib.fa_combine(C.byref(a), C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)))


# ---- the raw ops (namespace flash_attn_amd), with fake implementations: torch.compile / export trace through them without graph breaks -----------------
def _combine_impl(out_partial: torch.Tensor, lse_partial: torch.Tensor, out: Optional[torch.Tensor], out_dtype: Optional[torch.dtype],
                  return_lse: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (out, or an empty tensor when `out` was given and written; lse as the (.., L, H) view of a contiguous (.., H, L) tensor, or an empty tensor)."""
    packed = out_partial.dim() == 4
    n = out_partial.shape[0]
    shape = tuple(out_partial.shape[1:])
    ret_out = out is None
    if out is None:
        out = torch.empty(shape, dtype=out_dtype if out_dtype is not None else out_partial.dtype, device=out_partial.device)
    lse = None
    if return_lse:
        lse = torch.empty(shape[:-3] + (shape[-2], shape[-3]), dtype=torch.float32, device=out_partial.device).transpose(-1, -2)
    if packed:
        total, h, d = shape
        src = (out_partial, lse_partial, n, (out_partial.stride(0), 0, out_partial.stride(1), out_partial.stride(2)),
               (lse_partial.stride(0), 0, lse_partial.stride(1), lse_partial.stride(2)))
        _launch([src], out, lse, 1, total, h, d, (0, out.stride(0), out.stride(1)), (0,) + tuple(lse.stride()) if return_lse else None, -1)
    else:
        b, l, h, d = shape
        src = (out_partial, lse_partial, n, tuple(out_partial.stride()[:4]), tuple(lse_partial.stride()))
        _launch([src], out, lse, b, l, h, d, tuple(out.stride()[:3]), tuple(lse.stride()) if return_lse else None, -1)
    empty = out.new_empty((0,))
    return (out if ret_out else empty), (lse if return_lse else torch.empty((0,), dtype=torch.float32, device=out.device))


def _combine_fake(out_partial, lse_partial, out, out_dtype, return_lse):
    shape = tuple(out_partial.shape[1:])
    dev = out_partial.device
    o = (torch.empty(shape, dtype=out_dtype if out_dtype is not None else out_partial.dtype, device=dev) if out is None
         else torch.empty((0,), dtype=out.dtype, device=dev))
    lse = (torch.empty(shape[:-3] + (shape[-2], shape[-3]), dtype=torch.float32, device=dev).transpose(-1, -2) if return_lse
           else torch.empty((0,), dtype=torch.float32, device=dev))
    return o, lse


def _merge_impl(out_a: torch.Tensor, lse_a: torch.Tensor, out_b: torch.Tensor, lse_b: torch.Tensor, out: Optional[torch.Tensor],
                lse: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (out, lse): each a fresh tensor, or an empty one where the argument was given and written."""
    ret_out, ret_lse = out is None, lse is None
    if out is None:
        out = torch.empty(out_a.shape, dtype=out_a.dtype, device=out_a.device)
    if lse is None:
        lse = torch.empty(lse_a.shape, dtype=torch.float32, device=out_a.device)
    if out_a.dim() == 3:   # (total, H, D) / (H, total)
        total, h, d = out_a.shape
        b, s = 1, total
        ost = lambda t: (0, 0, t.stride(0), t.stride(1))
        lst = lambda t: (0, 0, t.stride(1), t.stride(0))
    else:                  # (B, S, H, D) / (B, H, S)
        b, s, h, d = out_a.shape
        ost = lambda t: (0, t.stride(0), t.stride(1), t.stride(2))
        lst = lambda t: (0, t.stride(0), t.stride(2), t.stride(1))
    _launch([(out_a, lse_a, 1, ost(out_a), lst(lse_a)), (out_b, lse_b, 1, ost(out_b), lst(lse_b))], out, lse, b, s, h, d, ost(out)[1:], lst(lse)[1:], +1)
    return (out if ret_out else out.new_empty((0,))), (lse if ret_lse else lse.new_empty((0,)))


def _merge_fake(out_a, lse_a, out_b, lse_b, out, lse):
    dev = out_a.device
    return (torch.empty(out_a.shape if out is None else (0,), dtype=out_a.dtype if out is None else out.dtype, device=dev),
            torch.empty(lse_a.shape if lse is None else (0,), dtype=torch.float32, device=dev))


def _register(name, impl, fake, mutates):
    op = torch.library.custom_op(f"flash_attn_amd::{name}", impl, mutates_args=mutates, device_types="cuda")
    op.register_fake(fake)
    return getattr(torch.ops.flash_attn_amd, name)


_flash_attn_combine = _register("_flash_attn_combine", _combine_impl, _combine_fake, ("out",))
_merge_attn_states = _register("_merge_attn_states", _merge_impl, _merge_fake, ("out", "lse"))


# ---- the public functions ----------------------------------------------------------------------------------------------------------------------------
def flash_attn_combine(out_partial: torch.Tensor, lse_partial: torch.Tensor, out: Optional[torch.Tensor] = None,
                       out_dtype: Optional[torch.dtype] = None, *, return_lse: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """FA3's flash_attn_combine: merge the S splits of a split-KV attention.

    out_partial: (S, B, L, H, D), or (S, total, H, D) for the packed form; fp32, bf16 or fp16; any view with a contiguous last dimension, 16-byte
    aligned data and strides that are multiples of 16 bytes.  lse_partial: fp32 (S, B, L, H) / (S, total, H), any strides (FA3 hands over the
    transpose of an (S, B, H, L) tensor).  S <= 256, D % 8 == 0, D <= 512.  A split whose lse is -inf (or +inf) is empty and its out_partial row is
    not read.  `out`: (B, L, H, D) / (total, H, D), written in place; otherwise a new tensor of `out_dtype` (default: out_partial's dtype).

    Returns (out, lse): lse is the (B, L, H) / (total, H) transposed view of a contiguous (B, H, L) / (H, total) fp32 tensor -- FA3's return, and
    `lse.transpose(-1, -2)` is this package's native lse layout; None with return_lse=False.  A row with no live split has out = 0, lse = -inf."""
    fn = "flash_attn_combine"
    _refuse_grad(fn, out_partial, lse_partial, out)
    if out_partial.dim() not in (4, 5) or lse_partial.dim() != out_partial.dim() - 1:
        raise RuntimeError(f"{fn}: out_partial must be (num_splits, batch, seqlen, heads, head_size) or (num_splits, total, heads, head_size), "
                           "and lse_partial the same without the last dimension")
    if tuple(lse_partial.shape) != tuple(out_partial.shape[:-1]):
        raise RuntimeError(f"{fn}: lse_partial must have shape {tuple(out_partial.shape[:-1])}, got {tuple(lse_partial.shape)}")
    if out_partial.dtype not in _DTYPES:
        raise RuntimeError(f"{fn}: out_partial must be fp32, bf16 or fp16 (got {out_partial.dtype})")
    if lse_partial.dtype != torch.float32:
        raise RuntimeError(f"{fn}: lse_partial must be fp32 (got {lse_partial.dtype})")
    if out_dtype is not None and out_dtype not in _DTYPES:
        raise RuntimeError(f"{fn}: out_dtype must be fp32, bf16 or fp16 (got {out_dtype})")
    _same_device(fn, out_partial, lse_partial, out)
    n, d = out_partial.shape[0], out_partial.shape[-1]
    if n < 1 or n > _c.FA_COMBINE_MAX_SPLITS:
        raise RuntimeError(f"{fn}: num_splits must be in [1, {_c.FA_COMBINE_MAX_SPLITS}] (got {n})")
    if d % 8 != 0 or d < 8 or d > 512:
        raise RuntimeError(f"{fn}: head_size must be a multiple of 8 in [8, 512] (got {d})")
    if out_partial.stride(-1) != 1:
        raise RuntimeError(f"{fn}: out_partial must have a contiguous last dimension")
    if out is not None:
        if tuple(out.shape) != tuple(out_partial.shape[1:]) or out.dtype not in _DTYPES or out.stride(-1) != 1:
            raise RuntimeError(f"{fn}: out must have shape {tuple(out_partial.shape[1:])}, dtype fp32 / bf16 / fp16 and a contiguous last dimension")
        if out_dtype is not None and out.dtype != out_dtype:
            raise RuntimeError(f"{fn}: out has dtype {out.dtype} but out_dtype is {out_dtype}")
    o, lse = _flash_attn_combine(out_partial, lse_partial, out, out_dtype, return_lse)
    return (o if out is None else out), (lse if return_lse else None)


def merge_attn_states(out_a: torch.Tensor, lse_a: torch.Tensor, out_b: torch.Tensor, lse_b: torch.Tensor, *, out: Optional[torch.Tensor] = None,
                      lse: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge two attention results over disjoint key sets, in this package's own layouts.

    out_a / out_b: (B, S, H, D) with lse_a / lse_b (B, H, S), or (total, H, D) with (H, total): what flash_attn_func(..., return_attn_probs=True),
    flash_attn_varlen_func and flash_attn_with_kvcache(..., return_softmax_lse=True) return, or views of those (row slices, batch slices) with a
    contiguous last dimension of out, 16-byte aligned data and out strides that are multiples of 16 bytes.  out_a and out_b are independently fp32, bf16
    or fp16; lse is fp32.  A row whose lse is +inf (no visible key; or -inf) on one side takes the other side exactly and that side's out row is not
    read; +inf on both sides gives out = 0, lse = +inf.

    `out` / `lse`: written in place; otherwise new contiguous tensors (out in out_a's dtype).  `out=out_a, lse=lse_a` is the in-place running merge.
    Returns (out, lse)."""
    fn = "merge_attn_states"
    _refuse_grad(fn, out_a, lse_a, out_b, lse_b, out, lse)
    if out_a.dim() not in (3, 4):
        raise RuntimeError(f"{fn}: out_a must be (batch, seqlen, heads, head_size) or (total, heads, head_size)")
    lse_shape = tuple(out_a.shape[:-3]) + (out_a.shape[-2], out_a.shape[-3])
    for name, o, l in (("a", out_a, lse_a), ("b", out_b, lse_b), ("", out, lse)):
        oname, lname = ("out_" + name, "lse_" + name) if name else ("out", "lse")
        if o is not None:
            if tuple(o.shape) != tuple(out_a.shape):
                raise RuntimeError(f"{fn}: {oname} must have the shape of out_a {tuple(out_a.shape)}, got {tuple(o.shape)}")
            if o.dtype not in _DTYPES:
                raise RuntimeError(f"{fn}: {oname} must be fp32, bf16 or fp16 (got {o.dtype})")
            if o.stride(-1) != 1:
                raise RuntimeError(f"{fn}: {oname} must have a contiguous last dimension")
        if l is not None:
            if tuple(l.shape) != lse_shape:
                raise RuntimeError(f"{fn}: {lname} must have shape (.., heads, seqlen) = {lse_shape}, got {tuple(l.shape)}")
            if l.dtype != torch.float32:
                raise RuntimeError(f"{fn}: {lname} must be fp32 (got {l.dtype})")
    _same_device(fn, out_a, lse_a, out_b, lse_b, out, lse)
    d = out_a.shape[-1]
    if d % 8 != 0 or d < 8 or d > 512:
        raise RuntimeError(f"{fn}: head_size must be a multiple of 8 in [8, 512] (got {d})")
    o, l = _merge_attn_states(out_a, lse_a, out_b, lse_b, out, lse)
    return (o if out is None else out), (l if lse is None else lse)
