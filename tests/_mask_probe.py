"""Exact visibility probe of the attention kernels' masks (test infrastructure only; a plain helper, not a conftest).

With q = 0 every score is exactly 0 whatever K holds, so P is exactly uniform over the visible keys of a row: P_ij = 1 / n_i.  Coded V / dO / K then turn
every output element into a small integer count (or a sum of a few terms of size 1) that moves by at least 0.5 when one (row, key) pair too many or too few is
visible.  The expected sets come from the oracle (normalize_window + visible_mask); nothing here is taken from the code under test.

  forward   V holds 0/1 codes in two halves of its columns, W = Dv / 2: fine c = j mod W, coarse c = W + (j // 16) mod W.
            count:    |exp(lse_i) - n_i| < 0.25, lse_i = +inf exactly where n_i = 0, and those rows of out exactly 0
            identity: |out[i, c] * n_i - #{visible j whose code has column c set}| < 0.25
  dV        v = 0 (so dP = dS = 0: dQ and dK exactly 0), dO[i, c_i] = 2^ceil(log2 n_i) in one column per row, c_i = (i + 7 g) mod Dv for head g of a group;
            dV[j, c] = sum over the rows that see j with c_i = c of 2^e_i / n_i, every term in [1, 2); against the same sum in fp64, < 0.25
  dQ        dO_i = e_0, v_j = a_j e_0 (a_j = +-1), k_j = e_(j mod D): n_i dQ[i, c] / scale = sum over visible j = c (mod D) of (a_j - delta_i), delta_i = the mean
            of a over the row's keys as the dtype holds it in out; two sign codes, (-1)^j and (-1)^(j // 2); < 0.25.  dK exactly 0 (q = 0).

THE CAP: no probed element sums more than 16 terms.  It is a condition on the reference, asserted before anything runs: with at most 16 terms the roundings of
P / dS and of the outputs of ONE kernel stay below 0.125 in bf16 (16 terms x 2^-9 x 2, plus the output's own 2^-9 x 16), half of the threshold, while a wrong
pair moves an element by at least 0.5.  (Where the dK/dV kernels split a GQA group, each partial dV is rounded to the dtype once more before the sum: up to
gs x 2^-9 x 16 on top, measured 0.147 at worst -- still under the threshold, but not inside this bound.)  Shapes that exceed the cap are split into PASSES -- key ranges of 16 W (forward), 16 D (dQ) keys, row ranges of 16 Dv / ratio rows
(dV) -- by zeroing the code of everything outside the pass; the passes ride on the (batch, kv head) slots of one call, or on several calls."""
from __future__ import annotations

import functools

import torch

from oracle import attention_oracle as orc

THRESHOLD = 0.25
CAP = 16
SCALE = 0.125   # passed explicitly: exact, and no kernel sees D ** -0.5

# (Sq, Sk): the smallest shapes that cross every block size in use -- 32 / 64 / 128 / 256 rows, 64-key tiles, 256-key blocks
SHAPES = [(1, 130), (65, 65), (128, 128), (129, 257), (257, 129), (320, 576), (576, 320), (513, 513), (1024, 1024), (300, 1100)]
# (causal, wl, wr)
MASKS = [(False, -1, -1), (True, -1, -1)] + [(False, wl, wr) for wl, wr in
                                             ((0, 0), (63, 0), (64, 0), (65, 0), (0, 64), (-1, 17), (17, -1), (100, 50), (255, 256), (300, 0))]
PACKED_LENS_Q = [257, 33, 0, 128, 1, 300]
PACKED_LENS_K = [257, 65, 5, 300, 77, 129]
PACKED_SEQUSED_K = [40, 65, 5, 300, 77, 10]   # seqused_k shortening entries 0 and 5
CACHE_LENS = [0, 1, 5, 64, 333, 1024]
CACHE_SQ = [1, 5, 33, 77, 130]
CACHE_MASKS = [(True, -1, -1), (False, 64, 0), (False, 200, -1)]


def mask_name(m):
    return "causal" if m[0] else ("none" if (m[1], m[2]) == (-1, -1) else "w(%d,%d)" % (m[1], m[2]))


@functools.lru_cache(maxsize=None)
def _mask_cpu(sq, sk, causal, wl, wr, max_seqlen_k):
    _, nl, nr = orc.normalize_window(sq, sk if max_seqlen_k is None else max_seqlen_k, causal, wl, wr)
    return torch.from_numpy(orc.visible_mask(sq, sk, nl, nr))


@functools.lru_cache(maxsize=None)
def visible(sq, sk, mask, max_seqlen_k=None, device="cpu"):
    """bool (Sq, Sk) of the oracle: mask = (causal, wl, wr), normalised by this call's own Sk or by max_seqlen_k (one sequence of a packed batch)."""
    return _mask_cpu(sq, sk, bool(mask[0]), int(mask[1]), int(mask[2]), max_seqlen_k).to(device)


def clear_caches():
    """Drop the cached masks, codes and expected sets (they live on the device the caller named)."""
    for fn in (_mask_cpu, visible, fwd_codes, _dv_probe, _dq_probe):
        fn.cache_clear()


def _assert_cap(terms, what):
    worst = int(terms.max()) if terms.numel() else 0
    assert worst <= CAP, f"mask probe: {what} would sum {worst} terms in one element (cap {CAP}): split into more passes"


def slot_passes(n_passes, b, hk, call=0):
    """(B, Hk) long: the pass each (batch, kv head) slot of call number `call` carries; n_calls(n_passes, B * Hk) calls cover all passes."""
    s = torch.arange(b * hk).reshape(b, hk)
    return (call * b * hk + s) % n_passes


def n_calls(n_passes, slots):
    return (n_passes + slots - 1) // slots


# ---------------------------------------------------------------- forward ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fwd_codes(sk, dv, device="cpu"):
    """(passes, Sk, Dv) fp32 0/1: the fine code in columns [0, W), the coarse code in [W, 2 W), W = Dv / 2; pass p codes the keys [16 W p, 16 W (p + 1))."""
    w = dv // 2
    n_p = max(1, -(-sk // (CAP * w)))
    j = torch.arange(sk)
    codes = torch.zeros(n_p, sk, dv)
    if sk:
        codes[j // (CAP * w), j, j % w] = 1.0
        codes[j // (CAP * w), j, w + (j // 16) % w] = 1.0
    return codes.to(device)


def fwd_expected(vis, codes):
    """(passes, Sq, Dv) fp32 integer counts of a row's visible keys per code column (exact in fp32), cap asserted."""
    exp = torch.einsum("ij,pjc->pic", vis.float(), codes)
    _assert_cap(exp, "the forward's count per code column")
    return exp


def fwd_values(codes, pass_of, dtype):
    """V of one call (B, Sk, Hk, Dv) from the codes and slot_passes()."""
    return codes[pass_of.to(codes.device)].permute(0, 2, 1, 3).contiguous().to(dtype)   # (B, Hk, Sk, Dv) -> (B, Sk, Hk, Dv)


def fwd_check(out, lse, vis, exp, pass_of_head):
    """One batch entry: out (Sq, H, Dv), lse (H, Sq), vis (Sq, Sk), exp = fwd_expected, pass_of_head (H,) long.
    -> dict of 0-dim tensors: count / fine / coarse = worst deviation, exact = number of violated exact rules (no host sync here)."""
    n = vis.sum(1).double()
    live = n > 0
    e = exp[pass_of_head.to(exp.device)].double()                         # (H, Sq, Dv)
    dev = (out.permute(1, 0, 2).double() * n[None, :, None] - e).abs()
    dev = torch.nan_to_num(dev, nan=float("inf"))
    w = out.shape[-1] // 2
    cnt = torch.nan_to_num((torch.exp(lse.double()) - n[None]).abs(), nan=float("inf"), posinf=float("inf"))
    cnt = torch.where(live[None], cnt, torch.zeros_like(cnt))
    dead = ~live
    exact = (lse[:, dead] != float("inf")).sum() + (out[dead] != 0).sum() + torch.isnan(out[dead].float()).sum()
    z = out.new_zeros((), dtype=torch.float64)
    return {"count": cnt.max() if cnt.numel() else z, "fine": dev[..., :w].max() if dev.numel() else z,
            "coarse": dev[..., w:].max() if dev.numel() else z, "exact": exact}


def fwd_failures(out, lse, vis, exp, pass_of_head, limit=4):
    """The slow path: [(message, head, [row])] of every violated rule of fwd_check (at most `limit` per rule)."""
    out, lse, vis, exp = out.detach().cpu(), lse.detach().cpu(), vis.cpu(), exp.cpu()
    n = vis.sum(1)
    w = out.shape[-1] // 2
    fails = []
    for h in range(out.shape[1]):
        e = exp[int(pass_of_head[h])].double()
        got = out[:, h].double() * n[:, None].double()
        bad = torch.nonzero(~((got - e).abs() < THRESHOLD))
        for i, c in bad[:limit].tolist():
            cls = "fine j %% %d == %d" % (w, c) if c < w else "coarse (j // 16) %% %d == %d" % (w, c - w)
            fails.append(("identity: head %d row %d (sees %d keys), key column class %s: expected count %d, got %.3f"
                          % (h, i, int(n[i]), cls, int(e[i, c]), float(got[i, c])), h, [i]))
        cnt = torch.exp(lse[h].double().clamp(max=50.0))
        dead = n == 0
        bad_cnt = ~dead & ~((cnt - n.double()).abs() < THRESHOLD)
        for i in torch.nonzero(bad_cnt).flatten()[:limit].tolist():
            fails.append(("count: head %d row %d: expected %d visible keys, exp(lse) = %.4f" % (h, i, int(n[i]), float(cnt[i])), h, [i]))
        bad_dead = dead & ((lse[h] != float("inf")) | (out[:, h] != 0).any(-1) | torch.isnan(out[:, h].float()).any(-1))
        for i in torch.nonzero(bad_dead).flatten()[:limit].tolist():
            fails.append(("exact: head %d row %d sees no key: lse must be +inf and out 0, got lse %r, max|out| %r"
                          % (h, i, float(lse[h, i]), float(out[i, h].float().abs().max())), h, [i]))
    return fails


# ---------------------------------------------------------------- backward: shared ----------------------------------------------------------------
def ref_lse(vis):
    """(Sq,) fp32: log n_i of the uniform softmax, +inf where the row sees no key -- what a correct forward hands the backward."""
    n = vis.sum(1).double()
    return torch.where(n > 0, torch.log(n.clamp(min=1)), torch.full_like(n, float("inf"))).float()


# ---------------------------------------------------------------- dV ----------------------------------------------------------------
def dv_offset(g, dv):
    return (7 * g) % dv


@functools.lru_cache(maxsize=None)
def _dv_probe(sq, sk, mask, max_seqlen_k, dv, ratio, device):
    vis = visible(sq, sk, mask, max_seqlen_k, device)
    n = vis.sum(1)
    e = torch.where(n > 0, torch.exp2(torch.ceil(torch.log2(n.clamp(min=1).double()))), torch.ones_like(n, dtype=torch.float64))   # 2^ceil(log2 n), 1 for empty rows
    assert sq == 0 or float(e.max()) <= 2048   # exact in bf16 and fp16
    chunk = max(1, CAP * dv // ratio)
    n_p = max(1, -(-sq // chunk))
    i = torch.arange(sq, device=device)
    dout = torch.zeros(n_p, ratio, sq, dv, dtype=torch.float64, device=device)
    for g in range(ratio):
        dout[i // chunk, g, i, (i + dv_offset(g, dv)) % dv] = e
    wgt = torch.where(n > 0, 1.0 / n.clamp(min=1).double(), torch.zeros_like(e))
    visd = vis.double()
    exp = torch.einsum("ij,pgic->pjc", visd * wgt[:, None], dout)                                  # (passes, Sk, Dv) fp64
    terms = torch.einsum("ij,pgic->pjc", visd * (n > 0)[:, None].double(), (dout > 0).double())
    _assert_cap(terms, "a dV element's rows")
    return dout.float(), exp


def dv_probe(sq, sk, mask, dv, ratio, max_seqlen_k=None, device="cpu"):
    """-> dO codes (passes, ratio, Sq, Dv) fp32 (powers of two: exact in bf16 and fp16) and the expected dV (passes, Sk, Dv) fp64; cap asserted."""
    return _dv_probe(sq, sk, tuple(mask), max_seqlen_k, dv, ratio, str(device))


def dv_dout(codes, pass_of, dtype):
    """dO of one call (B, Sq, H, Dv): head hk * ratio + g of batch b carries codes[pass_of[b, hk], g]."""
    c = codes[pass_of.to(codes.device)]                  # (B, Hk, ratio, Sq, Dv)
    b, hk, r, sq, dv = c.shape
    return c.reshape(b, hk * r, sq, dv).permute(0, 2, 1, 3).contiguous().to(dtype)


def dv_check(dv, exp, pass_of_hk):
    """One batch entry: dv (Sk, Hk, Dv) against exp[pass] -> worst deviation (0-dim)."""
    e = exp[pass_of_hk.to(exp.device)]                   # (Hk, Sk, Dv)
    dev = torch.nan_to_num((dv.permute(1, 0, 2).double() - e).abs(), nan=float("inf"))
    return dev.max() if dev.numel() else dv.new_zeros((), dtype=torch.float64)


def dv_failures(dv, exp, pass_of_hk, sq, ratio, limit=4):
    """[(message, kv head, candidate rows)]: the rows whose dO column is the failing one in that pass."""
    dv, exp = dv.detach().cpu(), exp.cpu()
    width = dv.shape[-1]
    chunk = max(1, CAP * width // ratio)
    fails = []
    for hk in range(dv.shape[1]):
        p = int(pass_of_hk[hk])
        bad = torch.nonzero(~((dv[:, hk].double() - exp[p]).abs() < THRESHOLD))
        for j, c in bad[:limit].tolist():
            rows = sorted({i for g in range(ratio) for i in range(p * chunk, min(sq, (p + 1) * chunk)) if (i + dv_offset(g, width)) % width == c})
            fails.append(("dV: kv head %d key %d, dO column class c_i == %d (rows %s of pass %d): expected %.4f, got %.4f"
                          % (hk, j, c, rows[:8], p, float(exp[p, j, c]), float(dv[j, hk, c])), hk, rows))
    return fails


# ---------------------------------------------------------------- dQ ----------------------------------------------------------------
def sign_code(sk, code, device="cpu"):
    j = torch.arange(sk, device=device)
    return 1.0 - 2.0 * (((j if code == 0 else j // 2) % 2).double())   # (-1)^j, (-1)^(j // 2)


@functools.lru_cache(maxsize=None)
def _dq_probe(sq, sk, mask, max_seqlen_k, d, code, dtype, device):
    vis = visible(sq, sk, mask, max_seqlen_k, device)
    visd = vis.double()
    n = vis.sum(1)
    a = sign_code(sk, code, device)
    abar = torch.where(n > 0, (visd @ a) / n.clamp(min=1).double(), torch.zeros(sq, dtype=torch.float64, device=device))
    o0 = abar.to(dtype)                                   # what out[:, 0] holds in the dtype; delta_i = dO . O = that value
    n_p = max(1, -(-sk // (CAP * d)))
    j = torch.arange(sk, device=device)
    kc = torch.zeros(n_p, sk, d, dtype=torch.float64, device=device)
    if sk:
        kc[j // (CAP * d), j, j % d] = 1.0
    exp = torch.einsum("ij,pjc->pic", visd * (a[None, :] - o0.double()[:, None]), kc)             # (passes, Sq, D) fp64
    _assert_cap(torch.einsum("ij,pjc->pic", visd, kc), "a dQ element's keys")
    return a, o0, kc.float(), exp


def dq_probe(sq, sk, mask, d, code, dtype, max_seqlen_k=None, device="cpu"):
    """-> a (Sk,) fp64 signs, o0 (Sq,) out[:, 0] in the dtype, K codes (passes, Sk, D) fp32, expected n_i dQ / scale (passes, Sq, D) fp64; cap asserted."""
    return _dq_probe(sq, sk, tuple(mask), max_seqlen_k, d, code, dtype, str(device))


def dq_keys(kc, pass_of, dtype):
    """K of one call (B, Sk, Hk, D)."""
    return kc[pass_of.to(kc.device)].permute(0, 2, 1, 3).contiguous().to(dtype)


def dq_check(dq, vis, exp, pass_of_head, scale=SCALE):
    """One batch entry: dq (Sq, H, D) -> (worst deviation of n_i dQ / scale, number of non-zero elements in rows that see no key)."""
    n = vis.sum(1).double()
    e = exp[pass_of_head.to(exp.device)]                 # (H, Sq, D)
    got = dq.permute(1, 0, 2).double() * (n / scale)[None, :, None]
    dev = torch.nan_to_num((got - e).abs(), nan=float("inf"))
    dead = n == 0
    exact = (dq[dead] != 0).sum() + torch.isnan(dq[dead].float()).sum()
    return (dev.max() if dev.numel() else dq.new_zeros((), dtype=torch.float64)), exact


def dq_failures(dq, vis, exp, pass_of_head, scale=SCALE, limit=4):
    dq, vis, exp = dq.detach().cpu(), vis.cpu(), exp.cpu()
    n = vis.sum(1)
    fails = []
    for h in range(dq.shape[1]):
        e = exp[int(pass_of_head[h])]
        got = dq[:, h].double() * (n.double() / scale)[:, None]
        ok = (got - e).abs() < THRESHOLD
        ok &= ~((n == 0)[:, None] & (dq[:, h] != 0))
        for i, c in torch.nonzero(~ok)[:limit].tolist():
            fails.append(("dQ: head %d row %d (sees %d keys), key column class j %% %d == %d: expected n dQ / scale %.4f, got %.4f"
                          % (h, i, int(n[i]), dq.shape[-1], c, float(e[i, c]), float(got[i, c])), h, [i]))
    return fails


def exact_zero(t):
    """0-dim: the number of elements that are not exactly 0 (a NaN counts)."""
    return (t != 0).sum() + torch.isnan(t.float()).sum()


# ---------------------------------------------------------------- the CPU stand-in ----------------------------------------------------------------
def standin_fwd(q, k, v, vis, scale=SCALE):
    """Plain torch attention of one batch entry with the kernels' roundings: q (Sq, H, D), k (Sk, Hk, D), v (Sk, Hk, Dv), vis (Sq, Sk) or per query head
    (H, Sq, Sk) -- the mask is an ARGUMENT, so that a wrong one can be put in.  P and out are rounded to the dtype.  -> out (Sq, H, Dv), lse (H, Sq) fp32."""
    dt = q.dtype
    h, g = q.shape[1], q.shape[1] // k.shape[1]
    vis = vis if vis.dim() == 3 else vis[None].expand(h, -1, -1)
    kf, vf = k.float().repeat_interleave(g, 1), v.float().repeat_interleave(g, 1)
    s = torch.einsum("ihd,jhd->hij", q.float(), kf) * scale
    s = s.masked_fill(~vis, float("-inf"))
    live = vis.any(-1)
    m = torch.where(live, s.max(-1).values, torch.zeros(()))
    p = torch.exp(s - m[..., None])
    l = p.sum(-1)
    lse = torch.where(live, m + torch.log(l.clamp(min=1e-30)), torch.full_like(m, float("inf")))
    pn = (p / l.clamp(min=1e-30)[..., None]).to(dt).float()
    out = torch.einsum("hij,jhc->ihc", pn, vf).to(dt)
    return out, lse


def standin_bwd(dout, q, k, v, out, lse, vis, scale=SCALE):
    """The backward of standin_fwd from a given out / lse: P and dS rounded to the dtype, fp32 sums, outputs rounded to the dtype -> dq, dk, dv."""
    dt = q.dtype
    h, hk = q.shape[1], k.shape[1]
    g = h // hk
    vis = vis if vis.dim() == 3 else vis[None].expand(h, -1, -1)
    kf, vf = k.float().repeat_interleave(g, 1), v.float().repeat_interleave(g, 1)
    s = torch.einsum("ihd,jhd->hij", q.float(), kf) * scale
    fin = torch.isfinite(lse)
    p = torch.where(vis & fin[..., None], torch.exp(s - torch.where(fin, lse, torch.zeros(()))[..., None]), torch.zeros(()))
    dof = dout.float()
    dv = torch.einsum("hij,ihc->jhc", p.to(dt).float(), dof)
    dp = torch.einsum("ihc,jhc->hij", dof, vf)
    delta = (dof * out.float()).sum(-1).transpose(0, 1)            # (H, Sq)
    ds = (p * (dp - delta[..., None])).to(dt).float()
    dq = (scale * torch.einsum("hij,jhd->ihd", ds, kf)).to(dt)
    dk = scale * torch.einsum("hij,ihd->jhd", ds, q.float())
    sk = k.shape[0]
    return dq, dk.reshape(sk, hk, g, -1).sum(2).to(dt), dv.reshape(sk, hk, g, -1).sum(2).to(dt)


# ---------------------------------------------------------------- mutants (wrong masks a kernel could compute) ----------------------------------------------------------------
def _window_mask(sq, sk, lo, hi, shift=None):
    """lo / hi: None = unbounded, else row i sees i + shift - lo <= j <= i + shift + hi (either may be negative here)."""
    i = torch.arange(sq)[:, None]
    j = torch.arange(sk)[None, :]
    shift = sk - sq if shift is None else shift
    vis = torch.ones(sq, sk, dtype=torch.bool)
    if hi is not None:
        vis &= j <= i + shift + hi
    if lo is not None:
        vis &= j >= i + shift - lo
    return vis


MUTANTS = ("wr+1", "wr-1", "wl+1", "wl-1", "top_left", "seam_tile", "last_key", "own_sk", "row_mod_sq", "row_div_g", "masked_row_key")


def mutant_mask(name, sq, sk, mask, max_seqlen_k=None, g=1):
    """The visible set a kernel with the named mistake would compute: bool (Sq, Sk), or (g, Sq, Sk) for the packed-row mutants (one mask per query head of a
    group).  None where the mutant provably equals the correct mask at this shape (nothing to perturb)."""
    _, wl, wr = orc.normalize_window(sq, sk if max_seqlen_k is None else max_seqlen_k, bool(mask[0]), int(mask[1]), int(mask[2]))
    good = visible(sq, sk, tuple(mask), max_seqlen_k)
    lo, hi = (None if wl < 0 else wl), (None if wr < 0 else wr)
    if name in ("wr+1", "wr-1"):
        return None if hi is None else _window_mask(sq, sk, lo, hi + (1 if name == "wr+1" else -1))
    if name in ("wl+1", "wl-1"):
        return None if lo is None else _window_mask(sq, sk, lo + (1 if name == "wl+1" else -1), hi)
    if name == "top_left":
        return None if (lo is None and hi is None) else _window_mask(sq, sk, lo, hi, shift=0)
    if name == "seam_tile":      # the rows of the second 256-row block lose the 64-key tile that holds the last key row 256 sees
        if sq <= 256 or not bool(good[256].any()):
            return None
        t = int(torch.nonzero(good[256]).max()) // 64
        m = good.clone()
        m[256:512, 64 * t:64 * t + 64] = False
        return m
    if name == "last_key":
        if sk == 0:
            return None
        m = good.clone()
        m[:, sk - 1] = False
        return m
    if name == "own_sk":         # a packed batch's window normalised by the sequence's own Sk instead of the batch's max_seqlen_k
        return None if max_seqlen_k is None else visible(sq, sk, tuple(mask))
    if name in ("row_mod_sq", "row_div_g"):
        if g <= 1 or sq <= 1:
            return None
        i, hh = torch.arange(sq)[None, :], torch.arange(g)[:, None]
        src = ((i * g + hh) % sq) if name == "row_mod_sq" else ((hh * sq + i) // g)   # query-major rows decoded as r % Sq; head-major rows decoded as r // g
        return good[src]                                                              # (g, Sq, Sk)
    if name == "masked_row_key":
        dead = torch.nonzero(~good.any(1))
        if sk == 0 or dead.numel() == 0:
            return None
        m = good.clone()
        m[int(dead[-1]), 0] = True                                                    # the last fully masked row sees key 0
        return m
    raise KeyError(name)
