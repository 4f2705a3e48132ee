"""Exact probe of the dropout kernels' keep sets (test infrastructure only; a plain helper, not a conftest).  Built on tests/_mask_probe.py.

With q = 0 every score is exactly 0 (a softcap leaves 0 at 0 with derivative 1, an ALiBi tensor of zeros adds 0: assert_uniform_scores checks it in fp64), so P
before dropout is exactly 1 / n_i over the n_i visible keys of row i, and dropout only multiplies the kept pairs by 1 / (1 - p).  The expected kept set is
kept = visible AND keep[b, h], keep from the host model of the stream (tests/_dropout_model.py: nothing is read from the code under test), per (batch, QUERY head).

  forward   V holds the mask probe's 0/1 codes (fine c = j mod W, coarse c = W + (j // 16) mod W, W = Dv / 2).  lse is that of the UN-dropped scores:
            count:    |exp(lse_i) - n_i| < 0.25, lse_i = +inf exactly where n_i = 0 and those rows of out exactly 0        (the mask probe's rules, unchanged)
            identity: |out[b, i, h, c] * n_i * (1 - p) - #{kept j whose code has column c set}| < 0.25
  dV        v = 0 (dP = dS = 0: dQ and dK exactly 0); dO[i, c_i] = s(p) * 2^ceil(log2 n_i) in one column per row, c_i = (i + 7 g) mod Dv for head g of a group,
            s(p) = the power of two nearest 1 - p.  dV[j, c] = sum over the rows with c_i = c that KEEP j of dO / (n_i (1 - p)); against that sum in fp64, < 0.25.
            Term range: [1, 2) * s / (1 - p), i.e. [1, 2) at p = 0.5, [1.2, 2.41) at 0.17, [1.25, 2.5) at 0.6, [0.98, 1.96) at 0.999, [1.001, 2.002) at 0.001.
  dQ        dO_i = s(p) e_0, v_j = a_j e_0 (a_j = (-1)^j), k_j = e_(j mod D); the kernel is handed the reference's own out (out[:, 0] = o_i = what the dtype holds
            of sum_kept a_j / (n_i (1 - p))) and lse = log n_i, so the backward is probed without the forward.  Expected
            n_i dQ[i, c] / scale = sum over VISIBLE j = c (mod D) of (keep_ij a_j s / (1 - p) - s o_i); < 0.25.  dK exactly 0 (q = 0).
            (dO is s(p) e_0 and not plain e_0 so that a kept term stays of size 1..2.5 at every p: at p = 0.999 an unscaled kept term is 1000 and
            its bf16 rounding alone is 4.)  Every visible key is a term, kept or dropped: a dropped pair still carries -s o_i.

THE CAP.  No element sums more than cap(p) = min(16, floor(32 / t(p))) terms, t(p) = 2 s / (1 - p) the largest term (2 at p = 0.5: cap 16; 13 at 0.17, 12 at 0.6,
16 at 0.999, 15 at 0.001), so that the sum of |terms| of an element is at most 32 at every p.  Asserted on the expected tensors before anything runs.
Keys (forward: 16 W, dQ: cap D) and rows (dV: cap Dv / ratio) are split into passes that ride on the (batch, kv head) slots; since the kept set differs per
query head, EVERY slot runs every pass (one call per pass), so every (batch, head, row, key) pair of a case is decoded.

THE THRESHOLD (0.25 for all three decoders) is derived, not tuned:
  * one flipped pair (kept <-> dropped) moves the forward's count by exactly 1, a dV element by one term >= 0.98 (>= 1 at p = 0.5), a dQ element by
    s / (1 - p) >= 0.98 (exactly 1 at p = 0.5).  Flips that only add or only remove keeps cannot cancel; two opposite flips in one forward element would have
    to share both code columns, which inside a pass of 16 W keys means the same key.
  * rounding, bf16 (half an ulp = 2^-9 of the binade's upper end): P (dV) or dS (dQ) is rounded once per term, at most 2^-9 x the sum of |terms| <= 2^-9 x 32
    = 0.0625; the output is rounded once, a value of at most 32: 0.0625.  Forward: at most 16 counts of 1 -> 16 x 2^-8 for a rounded P plus 16 x 2^-9 for
    out = 0.094.  So a correct kernel stays within 0.125 = half the threshold, a wrong pair leaves at least 0.98 - 0.125, and 0.25 lies between.  fp16 is 8x finer.
  * the CPU stand-in (P and dS rounded to the dtype, fp32 sums, outputs rounded once) with the model's keep set must stay within 0.125 on every case
    (tests/test_dropout_probe_cpu.py; profiles/dropout_probe_margins.txt holds the figures).
  * a split GQA group rounds each virtual head's partial dV to the dtype once more before the sum (fa_api.cpp bwd_gsplit_plan).  The partials are sums of
    positive terms and add up to at most 32; partial x is rounded by at most 2^-9 of its binade's upper end, i.e. by at most 2^-8 x, so all of them
    together by at most 2^-8 x 32 = 0.125 on top of the 0.125 above: a correct split kernel stays within 0.25, a wrong pair leaves at least
    0.98 - 0.25 = 0.73.  dV of a split run is therefore held to THRESHOLD_SPLIT = 0.375, between the two; its dQ and everything else keep 0.25.

ONE LIMIT.  A dropped-but-visible pair and an invisible pair differ in dQ only by s o_i, which can be near 0: the dQ probe decides kept against dropped, not
visible against invisible.  Visibility of the dropout variants is decided by the forward's count rule and by the dV probe (an invisible row contributes nothing,
a visible kept one a term >= 0.98; a visible dropped one is the keep decision itself)."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from tests import _dropout_model as dm
from tests import _mask_probe as mp

THRESHOLD = 0.25
THRESHOLD_SPLIT = 0.375   # dV of a split GQA group (see above)
SUM_BOUND = 32.0
SCALE = mp.SCALE


def scale_pow2(p):
    """s(p): the power of two nearest 1 - p (in the exponent)."""
    return 2.0 ** round(math.log2(dm.p_keep(p)))


def term_max(p):
    return 2.0 * scale_pow2(p) / dm.p_keep(p)


def cap_for(p):
    return min(mp.CAP, int(SUM_BOUND / term_max(p)))


# ---------------------------------------------------------------- the keep set ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bytes_np(seed, offset, h, b, sq, sk):
    return dm.rand_bytes(seed, offset, 1, h, sq, sk, b0=b)[0]


@functools.lru_cache(maxsize=None)
def model_bytes(seed, offset, h, b, sq, sk, device="cpu"):
    """uint8 (H, Sq, Sk) of batch entry / packed sequence b, rows and keys counted from 0."""
    return torch.from_numpy(_bytes_np(seed, offset, h, b, sq, sk)).to(device)


def model_keep(seed, offset, p, h, b, sq, sk, device="cpu"):
    return model_bytes(seed, offset, h, b, sq, sk, device) <= dm.threshold(p)


@functools.lru_cache(maxsize=None)
def rand_k(shape, dtype, device):
    g = torch.Generator().manual_seed(sum(shape))
    return torch.randn(shape, generator=g).to(device=device, dtype=dtype)


def clear_caches():
    for fn in (_bytes_np, model_bytes, rand_k, _dv_codes, _mutant_bytes):
        fn.cache_clear()


def assert_uniform_scores(q, k, softcap=0.0, alibi=None, scale=SCALE):
    """fp64: every score of q (Sq, H, D) against k (Sk, Hk, D) is exactly 0 after softcap and ALiBi (alibi: (H,) slopes or None)."""
    g = q.shape[1] // k.shape[1]
    s = torch.einsum("ihd,jhd->hij", q.double(), k.double().repeat_interleave(g, 1)) * scale
    if softcap:
        s = softcap * torch.tanh(s / softcap)
    if alibi is not None:
        i = torch.arange(q.shape[0], device=q.device)[:, None] + (k.shape[0] - q.shape[0])
        s = s - alibi.double()[:, None, None] * (i - torch.arange(k.shape[0], device=q.device)[None, :]).abs()[None].double()
    assert bool((s == 0).all()), "the probe needs exactly uniform scores"


class Problem:
    """One probed case: seqs = [(Sq, Sk)] per batch entry (equal for a fixed-length batch), the mask, p, rng = (seed, offset), the heads, dims and dtype;
    max_k: what the window of a packed batch is normalised by.  vis[b] (Sq, Sk) and keep[b] (H, Sq, Sk) are the EXPECTED sets."""

    def __init__(self, seqs, mask, p, rng, h, hk, d, dv, dtype, device="cpu", max_k=None):
        self.seqs, self.mask, self.p, self.rng, self.h, self.hk, self.d, self.dv, self.dtype, self.device = list(seqs), tuple(mask), p, tuple(rng), h, hk, d, dv, dtype, str(device)
        self.ratio, self.max_k, self.pk, self.s = h // hk, max_k, dm.p_keep(p), scale_pow2(p)
        self.vis = [mp.visible(nq, nk, self.mask, max_k, self.device) for nq, nk in self.seqs]
        self.keep = [model_keep(rng[0], rng[1], p, h, b, nq, nk, self.device) for b, (nq, nk) in enumerate(self.seqs)]
        self.live = [b for b, (nq, _) in enumerate(self.seqs) if nq > 0]

    def zeros(self, rows, heads, width):
        return torch.zeros(rows, heads, width, device=self.device, dtype=self.dtype)

    def lse(self, b):
        return mp.ref_lse(self.vis[b])[None].expand(self.h, -1).contiguous()


class Result:
    def __init__(self):
        self.devs, self.zeros = [], []   # [(decoder, 0-dim deviation, explain() -> [(message, b, head, [rows], key or None, column or None)])], [(0-dim count, what)]

    def add(self, decoder, value, explain):
        self.devs.append((decoder, value.detach().reshape(()), explain))

    def zero(self, count, what):
        self.zeros.append((count.reshape(()), what))

    def worst(self):
        """{decoder: float} and the number of violated exact rules (host sync)."""
        out = {}
        for dec, v, _ in self.devs:
            out[dec] = max(out.get(dec, 0.0), float(v))
        return out, sum(int(c) for c, _ in self.zeros)


def _passes_of(n_ps, hk, call):
    """[[pass of slot (b, kv head)]]: call number `call` of max(n_ps) calls; every slot runs every pass of its entry."""
    return [[(call + g + b) % n_p for g in range(hk)] for b, n_p in enumerate(n_ps)]


def _side(got, want):
    return "too high" if got > want else "too low"


# ---------------------------------------------------------------- forward ----------------------------------------------------------------
def fwd_expected(vis, keep, codes):
    """(H, passes, Sq, Dv) fp32 counts of a row's KEPT keys per code column; the cap is asserted on the visible set, which bounds every kept subset."""
    mp._assert_cap(torch.einsum("ij,pjc->pic", vis.float(), codes), "the forward's count per code column")
    return torch.einsum("hij,pjc->hpic", (vis[None] & keep).float(), codes)


def fwd_failures(out, lse, vis, exp_h, pk, b, limit=4):
    """The slow path: out (Sq, H, Dv), exp_h (H, Sq, Dv)."""
    out, lse, vis, exp_h = out.detach().cpu(), lse.detach().cpu(), vis.cpu(), exp_h.cpu()
    n = vis.sum(1)
    w = out.shape[-1] // 2
    fails = []
    for h in range(out.shape[1]):
        got = out[:, h].double() * n[:, None].double() * pk
        bad = torch.nonzero(~((got - exp_h[h].double()).abs() < THRESHOLD))
        for i, c in bad[:limit].tolist():
            cls = "fine j %% %d == %d" % (w, c) if c < w else "coarse (j // 16) %% %d == %d" % (w, c - w)
            fails.append(("identity: batch %d head %d row %d (sees %d keys), key column class %s: expected %d kept, got %.3f (%s)"
                          % (b, h, i, int(n[i]), cls, int(exp_h[h, i, c]), float(got[i, c]), _side(float(got[i, c]), float(exp_h[h, i, c]))), b, h, [i], None, c))
        cnt = torch.exp(lse[h].double().clamp(max=50.0))
        dead = n == 0
        for i in torch.nonzero(~dead & ~((cnt - n.double()).abs() < THRESHOLD)).flatten()[:limit].tolist():
            fails.append(("count: batch %d head %d row %d: expected %d visible keys (un-dropped), exp(lse) = %.4f (%s)"
                          % (b, h, i, int(n[i]), float(cnt[i]), _side(float(cnt[i]), float(n[i]))), b, h, [i], None, None))
        bad_dead = dead & ((lse[h] != float("inf")) | (out[:, h] != 0).any(-1) | torch.isnan(out[:, h].float()).any(-1))
        for i in torch.nonzero(bad_dead).flatten()[:limit].tolist():
            fails.append(("exact: batch %d head %d row %d sees no key: lse must be +inf and out 0" % (b, h, i), b, h, [i], None, None))
    return fails


def probe_fwd(pb, call, check_scores=None):
    """call(q_e, k_e, v_e) with per-entry lists q (Sq, H, D), k (Sk, Hk, D), v (Sk, Hk, Dv) -> [(out (Sq, H, Dv), lse (H, Sq))] per entry."""
    dev, res = pb.device, Result()
    codes = [mp.fwd_codes(nk, pb.dv, dev) for _, nk in pb.seqs]
    n_ps = [c.shape[0] for c in codes]
    exps = [fwd_expected(pb.vis[b], pb.keep[b], codes[b]) if b in pb.live else None for b in range(len(pb.seqs))]
    q_e = [pb.zeros(nq, pb.h, pb.d) for nq, _ in pb.seqs]
    k_e = [rand_k((nk, pb.hk, pb.d), pb.dtype, dev) for _, nk in pb.seqs]
    if check_scores is not None and pb.live:
        check_scores(q_e[pb.live[0]], k_e[pb.live[0]])
    heads = torch.arange(pb.h, device=dev)
    for cno in range(max(n_ps)):
        po = _passes_of(n_ps, pb.hk, cno)
        v_e = [codes[b][torch.tensor(po[b], device=dev)].permute(1, 0, 2).contiguous().to(pb.dtype) for b in range(len(pb.seqs))]
        outs = call(q_e, k_e, v_e)
        for b in pb.live:
            out, lse = outs[b]
            poh = torch.tensor(po[b], device=dev).repeat_interleave(pb.ratio)
            exp_h = exps[b][heads, poh]
            r = mp.fwd_check(out.double() * pb.pk, lse, pb.vis[b], exp_h, heads)
            ex = functools.partial(fwd_failures, out, lse, pb.vis[b], exp_h, pb.pk, b)
            for dec in ("count", "fine", "coarse"):
                res.add(dec, r[dec], ex if dec == "fine" else None)
            res.zero(r["exact"], "batch %d: rows without a visible key: lse must be +inf and out exactly 0" % b)
    return res


# ---------------------------------------------------------------- dV ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dv_codes(sq, sk, mask, max_k, dv, ratio, p, device):
    vis = mp.visible(sq, sk, mask, max_k, device)
    n = vis.sum(1)
    e = scale_pow2(p) * torch.where(n > 0, torch.exp2(torch.ceil(torch.log2(n.clamp(min=1).double()))), torch.ones_like(n, dtype=torch.float64))
    assert sq == 0 or (float(e.max()) <= 2048 and float(e.min()) >= 2.0 ** -12)   # exact in bf16 and fp16
    chunk = max(1, cap_for(p) * dv // ratio)
    n_p = max(1, -(-sq // chunk))
    i = torch.arange(sq, device=device)
    dout = torch.zeros(n_p, ratio, sq, dv, dtype=torch.float64, device=device)
    for g in range(ratio):
        dout[i // chunk, g, i, (i + mp.dv_offset(g, dv)) % dv] = e
    return dout, chunk


def dv_expected(vis, keep_g, dout, p):
    """keep_g (ratio, Sq, Sk) of one kv head's group, dout (passes, ratio, Sq, Dv) fp64 -> expected dV (passes, Sk, Dv) fp64; cap and sum bound asserted."""
    n = vis.sum(1)
    wgt = torch.where(n > 0, 1.0 / (n.clamp(min=1).double() * dm.p_keep(p)), torch.zeros(n.shape, dtype=torch.float64, device=vis.device))
    kept = (vis[None] & keep_g).double()
    exp = torch.einsum("gij,pgic->pjc", kept * wgt[None, :, None], dout)
    terms = torch.einsum("gij,pgic->pjc", kept * (n > 0)[None, :, None].double(), (dout > 0).double())
    assert (int(terms.max()) if terms.numel() else 0) <= cap_for(p), "dropout probe: a dV element would sum more than %d terms" % cap_for(p)
    assert (float(exp.max()) if exp.numel() else 0.0) <= SUM_BOUND, "dropout probe: a dV element exceeds the sum bound"
    return exp


def dv_failures(dv, exp_k, b, passes, chunk, sq, ratio, limit=4):
    """dv (Sk, Hk, Dv) against exp_k (Hk, Sk, Dv); passes[hk] = the pass the slot carried.  Names the candidate rows: those whose dO column is the failing one."""
    dv, exp_k = dv.detach().cpu(), exp_k.cpu()
    width = dv.shape[-1]
    fails = []
    for hk in range(dv.shape[1]):
        ps = int(passes[hk])
        bad = torch.nonzero(~((dv[:, hk].double() - exp_k[hk]).abs() < THRESHOLD))
        for j, c in bad[:limit].tolist():
            rows = sorted({i for g in range(ratio) for i in range(ps * chunk, min(sq, (ps + 1) * chunk)) if (i + mp.dv_offset(g, width)) % width == c})
            fails.append(("dV: batch %d kv head %d key %d, dO column class c_i == %d (rows %s of pass %d): expected %.4f, got %.4f (%s)"
                          % (b, hk, j, c, rows[:8], ps, float(exp_k[hk, j, c]), float(dv[j, hk, c]), _side(float(dv[j, hk, c]), float(exp_k[hk, j, c]))), b, hk, rows, j, c))
    return fails


def probe_dv(pb, call, check_scores=None):
    """call(dout_e, q_e, k_e, v_e, out_e, lse_e) -> [(dq, dk, dv)] per entry; lse (H, Sq)."""
    dev, res, nb = pb.device, Result(), len(pb.seqs)
    pr = [_dv_codes(nq, nk, pb.mask, pb.max_k, pb.dv, pb.ratio, pb.p, dev) for nq, nk in pb.seqs]
    n_ps = [c[0].shape[0] for c in pr]
    exps = []   # [b][hk] -> (passes, Sk, Dv)
    for b in range(nb):
        exps.append([dv_expected(pb.vis[b], pb.keep[b][g * pb.ratio:(g + 1) * pb.ratio], pr[b][0], pb.p) for g in range(pb.hk)] if b in pb.live else None)
    q_e = [pb.zeros(nq, pb.h, pb.d) for nq, _ in pb.seqs]
    k_e = [rand_k((nk, pb.hk, pb.d), pb.dtype, dev) for _, nk in pb.seqs]
    v_e = [pb.zeros(nk, pb.hk, pb.dv) for _, nk in pb.seqs]
    o_e = [pb.zeros(nq, pb.h, pb.dv) for nq, _ in pb.seqs]
    l_e = [pb.lse(b) for b in range(nb)]
    if check_scores is not None and pb.live:
        check_scores(q_e[pb.live[0]], k_e[pb.live[0]])
    for cno in range(max(n_ps)):
        po = _passes_of(n_ps, pb.hk, cno)
        do_e = []
        for b, (nq, _) in enumerate(pb.seqs):
            c = pr[b][0][torch.tensor(po[b], device=dev)]                         # (Hk, ratio, Sq, Dv)
            do_e.append(c.reshape(pb.h, nq, pb.dv).permute(1, 0, 2).contiguous().to(pb.dtype))
        grads = call(do_e, q_e, k_e, v_e, o_e, l_e)
        for b in range(nb):
            dq, dk, dvv = grads[b]
            res.zero(mp.exact_zero(dq), "batch %d: dQ of the dV probe (v = 0) must be exactly 0" % b)
            res.zero(mp.exact_zero(dk), "batch %d: dK of the dV probe (q = 0) must be exactly 0" % b)
            if b not in pb.live:
                res.zero(mp.exact_zero(dvv), "batch %d: dV of an entry without queries must be exactly 0" % b)
                continue
            exp_k = torch.stack([exps[b][g][po[b][g]] for g in range(pb.hk)])     # (Hk, Sk, Dv)
            dev_ = torch.nan_to_num((dvv.permute(1, 0, 2).double() - exp_k).abs(), nan=float("inf"))
            res.add("dv", dev_.max() if dev_.numel() else torch.zeros((), dtype=torch.float64, device=dev),
                    functools.partial(dv_failures, dvv, exp_k, b, po[b], pr[b][1], pb.seqs[b][0], pb.ratio))
    return res


# ---------------------------------------------------------------- dQ ----------------------------------------------------------------
def dq_build(vis, keep, d, p, dtype):
    """-> a (Sk,) fp64 signs, o0 (H, Sq) in the dtype (out[:, 0] of a correct forward), K codes (passes, Sk, D) fp32, expected n_i dQ / scale (H, passes, Sq, D)
    fp64; the cap (visible keys per element) and the sum bound asserted."""
    dev = vis.device
    sq, sk = vis.shape
    n = vis.sum(1)
    a = mp.sign_code(sk, 0, dev)
    pk, s = dm.p_keep(p), scale_pow2(p)
    kept = (vis[None] & keep).double()
    o0 = torch.where(n > 0, (kept @ a) / (n.clamp(min=1).double() * pk), torch.zeros(sq, dtype=torch.float64, device=dev)).to(dtype)
    width = cap_for(p) * d
    n_p = max(1, -(-sk // width))
    j = torch.arange(sk, device=dev)
    kc = torch.zeros(n_p, sk, d, dtype=torch.float64, device=dev)
    if sk:
        kc[j // width, j, j % d] = 1.0
    t = vis[None].double() * (kept * a[None, None, :] * (s / pk) - s * o0.double()[:, :, None])      # (H, Sq, Sk): every visible pair is a term
    exp = torch.einsum("hij,pjc->hpic", t, kc)
    cnt = torch.einsum("ij,pjc->pic", vis.double(), kc)
    assert (int(cnt.max()) if cnt.numel() else 0) <= cap_for(p), "dropout probe: a dQ element would sum more than %d terms" % cap_for(p)
    tot = torch.einsum("hij,pjc->hpic", t.abs(), kc)
    assert (float(tot.max()) if tot.numel() else 0.0) <= SUM_BOUND * (1 + 2.0 ** -7), "dropout probe: a dQ element exceeds the sum bound"   # (o0 is rounded: 2^-8 of slack)
    return a, o0, kc.float(), exp


def dq_failures(dq, vis, exp_h, b, scale=SCALE, limit=4):
    dq, vis, exp_h = dq.detach().cpu(), vis.cpu(), exp_h.cpu()
    n = vis.sum(1)
    fails = []
    for h in range(dq.shape[1]):
        got = dq[:, h].double() * (n.double() / scale)[:, None]
        ok = (got - exp_h[h]).abs() < THRESHOLD
        ok &= ~((n == 0)[:, None] & (dq[:, h] != 0))
        for i, c in torch.nonzero(~ok)[:limit].tolist():
            fails.append(("dQ: batch %d head %d row %d (sees %d keys), key column class j %% %d == %d: expected n dQ / scale %.4f, got %.4f (%s)"
                          % (b, h, i, int(n[i]), dq.shape[-1], c, float(exp_h[h, i, c]), float(got[i, c]), _side(float(got[i, c]), float(exp_h[h, i, c]))), b, h, [i], None, c))
    return fails


def probe_dq(pb, call, check_scores=None):
    """call(dout_e, q_e, k_e, v_e, out_e, lse_e) -> [(dq, dk, dv)] per entry."""
    dev, res, nb = pb.device, Result(), len(pb.seqs)
    built = [dq_build(pb.vis[b], pb.keep[b], pb.d, pb.p, pb.dtype) for b in range(nb)]
    n_ps = [x[2].shape[0] for x in built]
    q_e = [pb.zeros(nq, pb.h, pb.d) for nq, _ in pb.seqs]
    v_e, do_e, o_e = [], [], []
    for (nq, nk), (a, o0, _, _) in zip(pb.seqs, built):
        vv = pb.zeros(nk, pb.hk, pb.dv); vv[:, :, 0] = a.to(pb.dtype)[:, None]
        dd = pb.zeros(nq, pb.h, pb.dv); dd[:, :, 0] = pb.s
        oo = pb.zeros(nq, pb.h, pb.dv); oo[:, :, 0] = o0.transpose(0, 1)
        v_e.append(vv); do_e.append(dd); o_e.append(oo)
    l_e = [pb.lse(b) for b in range(nb)]
    heads = torch.arange(pb.h, device=dev)
    for cno in range(max(n_ps)):
        po = _passes_of(n_ps, pb.hk, cno)
        k_e = [built[b][2][torch.tensor(po[b], device=dev)].permute(1, 0, 2).contiguous().to(pb.dtype) for b in range(nb)]
        if check_scores is not None and pb.live and cno == 0:
            check_scores(q_e[pb.live[0]], k_e[pb.live[0]])
        grads = call(do_e, q_e, k_e, v_e, o_e, l_e)
        for b in range(nb):
            dq, dk, _ = grads[b]
            res.zero(mp.exact_zero(dk), "batch %d: dK of the dQ probe (q = 0) must be exactly 0" % b)
            if b not in pb.live:
                continue
            poh = torch.tensor(po[b], device=dev).repeat_interleave(pb.ratio)
            exp_h = built[b][3][heads, poh]
            dev_, ex = mp.dq_check(dq, pb.vis[b], exp_h, heads)
            res.add("dq", dev_, functools.partial(dq_failures, dq, pb.vis[b], exp_h, b))
            res.zero(ex, "batch %d: dQ of rows without a visible key must be exactly 0" % b)
    return res


# ---------------------------------------------------------------- the CPU stand-in ----------------------------------------------------------------
def standin_fwd(q, k, v, vis, keep, p, scale=SCALE):
    """Plain torch attention with dropout of one batch entry with the kernels' roundings; vis (Sq, Sk) and keep (H, Sq, Sk) are ARGUMENTS, so that a wrong
    one can be put in.  P is rounded to the dtype, the sum is fp32, out is rounded once.  -> out (Sq, H, Dv), lse (H, Sq) fp32 of the un-dropped scores."""
    dt = q.dtype
    h, g = q.shape[1], q.shape[1] // k.shape[1]
    kf, vf = k.float().repeat_interleave(g, 1), v.float().repeat_interleave(g, 1)
    s = (torch.einsum("ihd,jhd->hij", q.float(), kf) * scale).masked_fill(~vis[None], float("-inf"))
    live = vis.any(-1)[None].expand(h, -1)
    m = torch.where(live, s.max(-1).values, torch.zeros(()))
    pe = torch.exp(s - m[..., None])
    l = pe.sum(-1)
    lse = torch.where(live, m + torch.log(l.clamp(min=1e-30)), torch.full_like(m, float("inf")))
    pn = (pe / l.clamp(min=1e-30)[..., None]).to(dt).float() * keep.float()
    out = (torch.einsum("hij,jhc->ihc", pn, vf) * np.float32(1.0 / dm.p_keep(p))).to(dt)
    return out, lse


def standin_bwd(dout, q, k, v, out, lse, vis, keep, p, scale=SCALE):
    """The backward of standin_fwd from a given out / lse: P and dS rounded to the dtype, fp32 sums, outputs rounded once -> dq, dk, dv."""
    dt = q.dtype
    h, hk = q.shape[1], k.shape[1]
    g = h // hk
    rp = float(np.float32(1.0) / np.float32(dm.p_keep(p)))
    kf, vf = k.float().repeat_interleave(g, 1), v.float().repeat_interleave(g, 1)
    s = torch.einsum("ihd,jhd->hij", q.float(), kf) * scale
    fin = torch.isfinite(lse)
    pr = torch.where(vis[None] & fin[..., None], torch.exp(s - torch.where(fin, lse, torch.zeros(()))[..., None]), torch.zeros(()))
    kp = keep.float()
    dof = dout.float()
    dv = rp * torch.einsum("hij,ihc->jhc", (pr * kp).to(dt).float(), dof)
    dp = torch.einsum("ihc,jhc->hij", dof, vf)
    delta = (dof * out.float()).sum(-1).transpose(0, 1)
    ds = (pr * (dp * kp * rp - delta[..., None])).to(dt).float()
    dq = (scale * torch.einsum("hij,jhd->ihd", ds, kf)).to(dt)
    dk = scale * torch.einsum("hij,ihd->jhd", ds, q.float())
    sk = k.shape[0]
    return dq, dk.reshape(sk, hk, g, -1).sum(2).to(dt), dv.reshape(sk, hk, g, -1).sum(2).to(dt)


def standin_calls(pb, keep=None):
    """(fwd call, bwd call) for probe_fwd / probe_dv / probe_dq that run the stand-in with `keep` (default: the model's own)."""
    keep = pb.keep if keep is None else keep

    def fwd(q_e, k_e, v_e):
        return [standin_fwd(q_e[b], k_e[b], v_e[b], pb.vis[b], keep[b], pb.p) for b in range(len(pb.seqs))]

    def bwd(do_e, q_e, k_e, v_e, o_e, l_e):
        return [standin_bwd(do_e[b], q_e[b], k_e[b], v_e[b], o_e[b], l_e[b], pb.vis[b], keep[b], pb.p) for b in range(len(pb.seqs))]
    return fwd, bwd


# ---------------------------------------------------------------- mutants (wrong keep sets a kernel could draw) ----------------------------------------------------------------
MUTANTS = ("bytes_reversed", "group_tile_local", "group_bottom_right", "row_block_local", "packed_global_row_key", "packed_b0", "kv_head", "bh_hk",
           "counter_swapped", "strict_less", "offset_high_ignored", "seed_high_ignored", "fp64_threshold")


@functools.lru_cache(maxsize=None)
def _mutant_bytes(name, seed, offset, h, hk, b, sq, sk, row0, key0):
    u = np.uint64
    hh = np.arange(h, dtype=np.uint64)
    bh = u(b) * u(h) + hh
    i = np.arange(sq, dtype=np.uint64)
    j = np.arange(sk, dtype=np.uint64)
    jb = j                                   # what selects the byte of the word
    swap = False
    if name == "bytes_reversed":
        jb = u(3) - (j & u(3))
    elif name == "group_tile_local":
        j = j % u(64); jb = j
    elif name == "group_bottom_right":
        j = (j.astype(np.int64) + (sk - sq)).astype(np.uint64) & u(dm.M32); jb = j
    elif name == "row_block_local":
        i = i % u(256)
    elif name == "packed_global_row_key":
        i = i + u(row0); j = j + u(key0); jb = j
    elif name == "packed_b0":
        bh = hh
    elif name == "kv_head":
        bh = u(b) * u(h) + hh // u(h // hk)
    elif name == "bh_hk":
        bh = u(b) * u(hk) + hh
    elif name == "counter_swapped":
        swap = True
    elif name == "offset_high_ignored":
        offset &= dm.M32
    elif name == "seed_high_ignored":
        seed &= dm.M32
    key = dm.bh_key(seed, offset, bh)[:, None, None]
    ii, gg = i[None, :, None], (j >> u(2))[None, None, :]
    word = dm.drop_bytes(key, gg, ii) if swap else dm.drop_bytes(key, ii, gg)
    return ((word >> (u(8) * (jb & u(3)))[None, None, :]) & u(0xFF)).astype(np.uint8)


def mutant_keep(name, pb, cu_q=None, cu_k=None):
    """[bool (H, Sq, Sk)] per entry: the keep set a kernel with the named mistake would draw for the Problem; None where the mutant provably equals the model on
    every visible pair of the case (nothing to perturb).  cu_q / cu_k: the first global row / key of each entry of a packed batch."""
    seed, offset = pb.rng
    thr = dm.threshold(pb.p)
    out = []
    for b, (nq, nk) in enumerate(pb.seqs):
        if name in ("strict_less", "fp64_threshold"):
            byt = _bytes_np(seed, offset, pb.h, b, nq, nk)
            kp = (byt < thr) if name == "strict_less" else (byt <= math.floor(255.0 * (1.0 - pb.p)))
        else:
            if name in ("packed_global_row_key", "packed_b0") and cu_q is None:
                return None
            r0, k0 = (int(cu_q[b]), int(cu_k[b])) if cu_q is not None and name == "packed_global_row_key" else (0, 0)
            kp = _mutant_bytes(name, seed, offset, pb.h, pb.hk, b, nq, nk, r0, k0) <= thr
        out.append(torch.from_numpy(kp).to(pb.device))
    differs = any(bool(((out[b] != pb.keep[b]) & pb.vis[b][None]).any()) for b in pb.live)
    return out if differs else None
