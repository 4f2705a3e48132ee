"""CPU reference of the e4m3 quantisation (include/fa_gfx950_quant.h, "Semantics"): plain torch fp32 ops, nothing else.  Test infrastructure only."""
from __future__ import annotations

import torch

FP8 = torch.float8_e4m3fn


def quant_ref(x, hk, cu_seqlens=None, descale=None):
    """x: CPU bf16 / fp16 (B, S, H, D), or packed (total, H, D) with cu_seqlens (a list of B + 1 ints); descale: None (dynamic) or fp32 (B, hk)
    (static).  Returns (y float8_e4m3fn of x's shape, descale fp32 (B, hk))."""
    x = x.cpu()
    H, D = x.shape[-2:]
    r = H // hk
    B = x.shape[0] if cu_seqlens is None else len(cu_seqlens) - 1
    y = torch.empty(x.shape, dtype=FP8)
    ds_out = torch.ones(B, hk, dtype=torch.float32)
    for b in range(B):
        rows = x[b] if cu_seqlens is None else x[int(cu_seqlens[b]):int(cu_seqlens[b + 1])]
        yb = y[b] if cu_seqlens is None else y[int(cu_seqlens[b]):int(cu_seqlens[b + 1])]
        g = rows.float().reshape(rows.shape[0], hk, r * D)          # (S, hk, r * D): a KV head's group of query heads side by side
        if descale is not None:
            ds = descale[b].cpu().float().clone()
        elif rows.shape[0] == 0:
            ds = torch.ones(hk, dtype=torch.float32)
        else:
            amax = g.abs().amax(dim=(0, 2))
            ds = torch.where(amax > 0, amax / 448, torch.ones_like(amax))
        inv = 1 / ds
        q = (g * inv[None, :, None]).clamp(-448, 448).to(FP8)
        yb.view(torch.uint8).copy_(q.view(torch.uint8).reshape(rows.shape))
        ds_out[b] = ds
    return y, ds_out


def dequant(y, ds, cu_seqlens=None):
    """float(y) * descale of its group, fp32 (the consumers' indexing)."""
    y = y.cpu().float()
    hk = ds.shape[1]
    r = y.shape[-2] // hk
    d = ds.cpu().repeat_interleave(r, dim=1)                            # (B, H)
    if cu_seqlens is None:
        return y * d[:, None, :, None]
    out = torch.empty_like(y)
    for b in range(len(cu_seqlens) - 1):
        out[int(cu_seqlens[b]):int(cu_seqlens[b + 1])] = y[int(cu_seqlens[b]):int(cu_seqlens[b + 1])] * d[b][None, :, None]
    return out
