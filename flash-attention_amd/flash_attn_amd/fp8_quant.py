"""The producer side of the FP8 paths: bf16 / fp16 activations -> float8_e4m3fn tensors and fp32 (B, Hk) descales on the GPU
(libfa_gfx950_quant.so, include/fa_gfx950_quant.h), in the form flash_attn_func / flash_attn_varlen_func / flash_attn_with_kvcache take them.

    (q8, q_descale), = quantize_fp8(q, num_heads_k=Hk)                               # dynamic: descale = amax / 448 per (batch entry, KV head)
    (k8, _), (v8, _) = quantize_fp8(k=k, v=v, num_heads_k=Hk, k_descale=ks, v_descale=vs)   # static: the cache's scales, saturating
    kvcache_append_fp8(k_cache, v_cache, k, v, cache_seqlens, ks, vs)                # quantise new rows straight into an e4m3 cache

The checks read shapes and dtypes only; nothing synchronises with the host, so both calls can be captured in a HIP graph.  Forward only.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _cabi_quant as _q

_FP8 = torch.float8_e4m3fn
_DTYPES = {torch.float16: 0, torch.bfloat16: 1}   # FA_DTYPE_FP16 / FA_DTYPE_BF16


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _refuse_grad(fn: str, *ts) -> None:
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError(f"{fn} has no backward: call it under torch.no_grad() or on tensors that do not require grad")


def _check_descale(fn: str, name: str, t: torch.Tensor, batch: int, hk: int, device) -> None:
    if t.dtype != torch.float32 or tuple(t.shape) != (batch, hk) or t.device != device:
        raise RuntimeError(f"{fn}: {name} must be an fp32 tensor of shape (batch_size, num_heads_k) = ({batch}, {hk}) on the inputs' device")


def quantize_fp8(q: Optional[torch.Tensor] = None, k: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None, *, num_heads_k: int,
                 cu_seqlens_q: Optional[torch.Tensor] = None, cu_seqlens_k: Optional[torch.Tensor] = None,
                 q_descale: Optional[torch.Tensor] = None, k_descale: Optional[torch.Tensor] = None, v_descale: Optional[torch.Tensor] = None,
                 path: int = 0) -> Tuple[Tuple[torch.Tensor, torch.Tensor], ...]:
    """Quantise up to three bf16 / fp16 tensors to float8_e4m3fn in one call (one or two kernel launches for all of them).

    q / k / v: (B, S, heads, D), or packed (total, heads, D) with cu_seqlens_q (for q) / cu_seqlens_k (for k and v); any view with 16-byte aligned
    data and strides that are multiples of 8 elements; D % 16 == 0, heads % num_heads_k == 0.  One scale per (batch entry, KV head): the query
    heads of a GQA group share their KV head's.  A descale that is passed in (fp32 (B, num_heads_k), any strides) is READ -- static mode, values
    beyond 448 * descale saturate; otherwise it is computed as amax / 448 (1.0 for an all-zero or empty group) and returned.  Non-finite inputs
    are unspecified.  `path`: 0 picks from the shapes, 1 forces the two-pass kernels, 2 the one-launch kernel (refused for a group of more than
    16384 elements); the bytes do not depend on it.

    Returns one (fp8 tensor, descale) pair per tensor given, in q, k, v order; the fp8 tensors are contiguous."""
    fn = "quantize_fp8"
    slots = [(n, x, cu, ds) for n, x, cu, ds in (("q", q, cu_seqlens_q, q_descale), ("k", k, cu_seqlens_k, k_descale), ("v", v, cu_seqlens_k, v_descale)) if x is not None]
    if not slots:
        raise RuntimeError(f"{fn}: pass at least one of q, k, v")
    first = slots[0][1]
    _refuse_grad(fn, *(s[1] for s in slots))
    hk = int(num_heads_k)
    batch = None
    for name, x, cu, _ in slots:
        if not x.is_cuda or x.device != first.device:
            raise RuntimeError(f"{fn}: {name} must be on the same CUDA device as the other inputs")
        if x.dtype not in _DTYPES or x.dtype != first.dtype:
            raise RuntimeError(f"{fn}: the inputs must all be fp16 or all be bf16 (got {x.dtype} for {name})")
        if x.dim() != (3 if cu is not None else 4) or x.stride(-1) != 1:
            raise RuntimeError(f"{fn}: {name} must be (batch, seqlen, heads, head_size) -- or (total, heads, head_size) with cu_seqlens -- with a contiguous last dimension")
        if x.shape[-1] != first.shape[-1]:
            raise RuntimeError(f"{fn}: the inputs must share one head size")
        if cu is not None and (cu.dtype != torch.int32 or cu.dim() != 1 or not cu.is_contiguous() or cu.device != x.device or cu.numel() < 2):
            raise RuntimeError(f"{fn}: cu_seqlens must be a contiguous int32 tensor of shape (batch_size + 1) on the inputs' device")
        b = cu.numel() - 1 if cu is not None else x.shape[0]
        if batch is None:
            batch = b
        elif b != batch:
            raise RuntimeError(f"{fn}: the inputs must share one batch size (got {batch} and {b})")
    if batch <= 0 or hk <= 0:
        raise RuntimeError(f"{fn}: batch size and num_heads_k must be positive")
    a = _q.FaQuantParams()
    a.n_tensors, a.b, a.h_k, a.d, a.dtype, a.path = len(slots), batch, hk, first.shape[-1], _DTYPES[first.dtype], int(path)
    out = []
    for i, (name, x, cu, ds) in enumerate(slots):
        t = a.t[i]
        static = ds is not None
        if static:
            _check_descale(fn, name + "_descale", ds, batch, hk, x.device)
        else:
            ds = torch.empty((batch, hk), dtype=torch.float32, device=x.device)
        y = torch.empty(x.shape, dtype=_FP8, device=x.device)
        t.x, t.y, t.descale, t.cu_seqlens = _ptr(x), _ptr(y), _ptr(ds), _ptr(cu)
        if cu is None:
            t.x_batch_stride, t.x_row_stride, t.x_head_stride = x.stride(0), x.stride(1), x.stride(2)
            t.y_batch_stride, t.y_row_stride, t.y_head_stride = y.stride(0), y.stride(1), y.stride(2)
            t.rows = x.shape[1]
        else:
            t.x_row_stride, t.x_head_stride = x.stride(0), x.stride(1)
            t.y_row_stride, t.y_head_stride = y.stride(0), y.stride(1)
            t.rows = x.shape[0]
        t.descale_batch_stride, t.descale_head_stride = ds.stride(0), ds.stride(1)
        t.heads, t.is_static = x.shape[-2], int(static)
        out.append((y, ds))
    lib = _q.load()
    with torch.cuda.device(first.device):
        ws_bytes = lib.fa_quant_workspace_bytes(C.byref(a))
        if ws_bytes > 0:
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=first.device)
            a.workspace, a.workspace_bytes = _ptr(ws), ws_bytes
        _q.check(lib.fa_quant_e4m3(C.byref(a), _stream(first.device)))
    return tuple(out)


def kvcache_append_fp8(k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cache_seqlens: torch.Tensor,
                       k_descale: torch.Tensor, v_descale: torch.Tensor, cache_batch_idx: Optional[torch.Tensor] = None,
                       block_table: Optional[torch.Tensor] = None) -> None:
    """Quantise the new bf16 / fp16 k / v (B, S_new, Hk, D) with the cache's scales and write them, in place, into the float8_e4m3fn caches at rows
    cache_seqlens[b] .. cache_seqlens[b] + S_new - 1 of cache entry b (or cache_batch_idx[b], or the pages block_table[b] names): one launch, the bytes
    of quantize_fp8(static) followed by the fp8 append of flash_attn_with_kvcache.  k_descale / v_descale: fp32 (B, Hk), indexed by the batch entry of
    k -- flash_attn_with_kvcache's convention.  The caller keeps cache_seqlens[b] + S_new within the cache (nothing here reads device memory on the
    host).  Returns nothing."""
    fn = "kvcache_append_fp8"
    _refuse_grad(fn, k, v)
    for t in (k_cache, v_cache, k, v, cache_seqlens, k_descale, v_descale, cache_batch_idx, block_table):
        if t is not None and (not t.is_cuda or t.device != k.device):
            raise RuntimeError(f"{fn}: every tensor must be on the same CUDA device")
    if k_cache.dtype != _FP8 or v_cache.dtype != _FP8:
        raise RuntimeError(f"{fn}: k_cache and v_cache must have dtype torch.float8_e4m3fn")
    if k.dtype not in _DTYPES or v.dtype != k.dtype:
        raise RuntimeError(f"{fn}: k and v must both be fp16 or both be bf16")
    for t in (k_cache, v_cache, k, v):
        if t.dim() != 4 or t.stride(-1) != 1:
            raise RuntimeError(f"{fn}: k_cache, v_cache, k and v must be 4-D with a contiguous last dimension")
    B, s_new, Hk, D = k.shape
    if tuple(v.shape) != (B, s_new, Hk, D):
        raise RuntimeError(f"{fn}: k and v must have the same shape")
    if tuple(k_cache.shape) != tuple(v_cache.shape) or k_cache.shape[2] != Hk or k_cache.shape[3] != D:
        raise RuntimeError(f"{fn}: k_cache / v_cache must be (.., .., num_heads_k, head_size) = (.., .., {Hk}, {D}) and equal in shape")
    paged = block_table is not None
    if paged:
        if cache_batch_idx is not None:
            raise RuntimeError("Paged KVcache does not support cache_batch_idx")
        if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.stride(-1) != 1 or block_table.shape[0] != B:
            raise RuntimeError("block_table must be a 2-D int32 tensor (batch_size, max_num_blocks_per_seq) with a contiguous last dimension")
        capacity = block_table.shape[1] * k_cache.shape[1]
    else:
        if cache_batch_idx is None and k_cache.shape[0] != B:
            raise RuntimeError(f"{fn}: the cache's batch size must match k (or pass cache_batch_idx)")
        capacity = k_cache.shape[1]
    if s_new > capacity:
        raise RuntimeError("If key is supplied, it must have seqlen <= the seqlen of the KV cache")
    for nm, t in (("cache_seqlens", cache_seqlens), ("cache_batch_idx", cache_batch_idx)):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != (B,)):
            raise RuntimeError(f"{nm} must be a contiguous int32 tensor of shape (batch_size)")
    _check_descale(fn, "k_descale", k_descale, B, Hk, k.device)
    _check_descale(fn, "v_descale", v_descale, B, Hk, k.device)
    a = _q.FaQuantAppendParams()
    a.knew, a.vnew, a.kcache, a.vcache, a.k_descale, a.v_descale = _ptr(k), _ptr(v), _ptr(k_cache), _ptr(v_cache), _ptr(k_descale), _ptr(v_descale)
    for nm, t in (("knew", k), ("vnew", v), ("kcache", k_cache), ("vcache", v_cache)):
        setattr(a, nm + "_batch_stride", t.stride(0)); setattr(a, nm + "_row_stride", t.stride(1)); setattr(a, nm + "_head_stride", t.stride(2))
    a.k_descale_batch_stride, a.k_descale_head_stride = k_descale.stride(0), k_descale.stride(1)
    a.v_descale_batch_stride, a.v_descale_head_stride = v_descale.stride(0), v_descale.stride(1)
    a.seqlens_k, a.cache_batch_idx, a.block_table = _ptr(cache_seqlens), _ptr(cache_batch_idx), _ptr(block_table)
    a.block_table_batch_stride, a.page_block_size = (block_table.stride(0) if paged else 0), (k_cache.shape[1] if paged else 0)
    a.b, a.seqlen_new, a.h_k, a.d, a.dtype = B, s_new, Hk, D, _DTYPES[k.dtype]
    lib = _q.load()
    with torch.cuda.device(k.device):
        _q.check(lib.fa_quant_kvcache_append(C.byref(a), _stream(k.device)))
