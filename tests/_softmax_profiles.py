"""Inputs with a PRESCRIBED score profile, for the online-softmax rescale paths (test infrastructure only; a plain helper, not a conftest).

Every forward kernel defers its rescale: the running maximum m of a row moves only when a step's maximum exceeds it by more than FwdK::rescale_thr log2
units, l is scaled at once and O one step later.  On randn data that code runs at a row's first key and never again.  Here a list of TARGETS
(row, head, key, height) puts single keys of a chosen height (log2 units, the unit the kernels compare with the threshold) on chosen rows:

  target t owns channel c0 + t: q[row, head, c0 + t] = 1 and k[key, kv head, c0 + t] = what makes the key's whole score equal the height; no other row and no other
  key touches the channel, so targets are independent and the rows WITHOUT a target -- they share waves with rows that have one -- see the same scores, bit for bit,
  as in a call whose targets are removed.  The other channels hold a quiet randn background (score std BG = 0.25 log2 units: at 1 unit the background's own maximum eats
  the margin of a spike).  softmax_scale = 0.1875 / log2(e) is passed explicitly: scale * log2(e) = 0.1875 is exact in bf16 / fp16 / e4m3, so the once-rounded
  Q' = q * scale * log2(e) of the default numerics is exact on the target channels.  V is randn with four coded columns (+-4 by the parity of the key's 64-key block,
  by the key's half, by the parity of its 32-key step, by the key lying ahead of the tile-aligned fires): a block of keys that is lost or counted twice, or the
  part of a row ahead of a spike weighted wrongly, moves an element by far more than a rounding.

Kinds (thr = the threshold in force; `first` = the score of the row's first visible key, `prior` = the maximum of the visible keys before the target):
  fire    one key at prior + thr + 2 (a row's first visible key: FIRST_HEIGHT)              hold    one key at first + thr - 1: must not move m, P ~ 2^(thr - 1)
  twice   fire keys in two consecutive 32-key steps                                         stairs  +6 in each of four consecutive steps
  decoy   a key MASKED for its row, 3 above the fire it accompanies, in the same 32-key step
  tail    a fire at Sk - 1 where the 20 % condition below cannot hold (thr = 0): the factor is still pending in the epilogue, and dropping it shows without the condition
Conditions, asserted on the fp64 scores of the finished tensors before anything runs (check_conditions): every fire exceeds prior by >= thr + 0.5; every hold stays
<= first + thr - 0.5 (m >= first in every correct kernel: it does not move m); every decoy is invisible; for thr <= 8 the keys before a fire and the keys from it on
each hold >= 20 % of the row's softmax mass -- without that a doubled or dropped factor is invisible; it needs ~2^(thr + 1.5) keys ahead, which is why the
default-threshold shapes have 1100 keys and the thr = 0 ones 333.  Two exceptions, both forced by arithmetic: a fire at a row's first visible key has nothing before it,
and the SECOND growth of a `twice` at thr > 2 leaves 2^-(thr + 2) of everything before it -- there the condition is put on the first growth alone, and what makes a lost
first factor visible (mutant 5) is asserted instead: the mass before the pair, times the factor that would be lost, is >= 20 % of the row.

standin() is a torch emulation of the deferred, lagged update (32-key steps, Q' rounded once, P rounded to bf16 / fp16 / e4m3, fp32 m / l / O, the factor applied to
O one step late and in the epilogue) that takes a MUTANT: tests/test_softmax_profiles_cpu.py shows that it meets the GPU module's bounds on every case list and that every
mutant is reported.  LSE_BOUND is set once from that run (profiles/softmax_profiles.txt)."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from oracle import attention_oracle as orc

LOG2E = 1.4426950408889634
C = 0.1875                 # softmax_scale * log2(e), exact in every input dtype
SCALE = C / LOG2E
STEP = 32
BG = 0.25                  # std of the background scores, log2 units
FIRST_HEIGHT = 3.0         # a fire at a row's first visible key
# softcap of the profiles: the capped kernels fold 2 scale log2(e) / softcap = 0.375 / softcap into Q', and 24 makes that 2^-6, exact like 0.1875 (at softcap 30 the
# once-rounded Q' carries 2^-9 of a spike's raw score into LSE: 1e-2 in bf16, the property lse_tolerance() of tests/test_baseline_configs_gpu.py documents).  A capped
# score cannot exceed SOFTCAP * log2(e) = 34.6 log2 units: every height, the stairs' 25 and the decoys included, stays under it (build() asserts that).
SOFTCAP = 24.0
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "e4m3": torch.float8_e4m3fn}
# LSE against the fp64 oracle: 2 x the stand-in's worst deviation over every case list (measured 8.2e-4: 1.6e-3, profiles/softmax_profiles.txt), never below 2e-3; the e4m3
# families keep the relative rule of their own check functions.
LSE_BOUND = 2e-3
MUTANTS = ("o_never", "o_twice", "l_not", "epilogue_drop", "overwrite", "group_factor", "mask_lost", "prev_tile", "first_no_grow")


def window_of(sq, sk, mask, alibi=False):
    causal, wl, wr = orc.normalize_window(sq, sk, bool(mask[0]), int(mask[1]), int(mask[2]), alibi)
    return wl, wr


def bounds(sq, sk, mask, alibi=False):
    """(lo, hi) int64 (Sq,): the visible keys of row i are lo[i] .. hi[i] (empty where lo > hi)."""
    wl, wr = window_of(sq, sk, mask, alibi)
    i = np.arange(sq, dtype=np.int64) + (sk - sq)
    hi = np.full(sq, sk - 1, dtype=np.int64) if wr < 0 else np.minimum(sk - 1, i + wr)
    lo = np.zeros(sq, dtype=np.int64) if wl < 0 else np.maximum(0, i - wl)
    return lo, hi


# ---------------------------------------------------------------- plans: where the targets go ----------------------------------------------------------------
def make_plan(sq, sk, mask, thr, heads, edges=(), kinds=("first", "tile_first", "tile_last", "last_key", "diag", "win_lo", "hold", "twice", "stairs"), alibi=False, slack=0.0):
    """[(kind, row, head, [keys], decoy key or None)] for one batch entry.  Rows are searched in a fixed spread order; a placement that no row can take at this shape and
    mask (a diagonal without a right bound, a fire with too few keys ahead) is left out -- placements_of() says what a plan holds, the case lists assert what they need.
    edges: first keys of KV splits (a fire goes on the largest, a hold on the key before it)."""
    lo, hi = bounds(sq, sk, mask, alibi)
    wl, wr = window_of(sq, sk, mask, alibi)
    used, r_used, plan = set(), {}, []
    order = sorted(range(sq), key=lambda i: (i * 37 + 5) % max(sq, 1))
    k_a = max(128, (int(0.72 * sk) // 128) * 128)

    def take(kind, key_of, span=1, stride=STEP, decoy_of=None, before=False, past=False):
        for i, hd in [(i, (len(plan) + r) % heads) for r in range(heads) for i in order]:   # (a row per target while there are rows; then the row's other heads)
            if (i, hd) in used or (r_used.get(i, 0) and sq >= 64):
                continue
            k0 = key_of(i)
            if k0 is None:
                continue
            keys = [k0 + stride * j for j in range(span)]
            if keys[0] < lo[i] or keys[-1] > hi[i]:
                continue
            if before and thr <= 8:                            # the 20 % condition, from the key counts: the spike weighs ~2^(thr + 2.8) background keys
                n_b, n_a = keys[0] - lo[i], (STEP - 1 if span > 1 else hi[i] - keys[0]) + 2.0 ** (thr + 2.8 + slack)
                if min(n_b, n_a) < 0.24 * (n_b + n_a):
                    continue
            dk = decoy_of(i) if decoy_of else None
            if decoy_of and (dk is None or dk < 0 or (dk >= sk and not past) or lo[i] <= dk <= hi[i] or dk // STEP != keys[0] // STEP):
                continue
            used.add((i, hd))
            r_used[i] = 1
            plan.append((kind, i, hd, keys, dk))
            return True
        return False

    for kind in kinds:
        if kind == "first":                                   # the thr_l = -inf start: the row's first visible key is its largest
            take("fire", lambda i: int(lo[i]) if hi[i] - lo[i] >= 40 else None)
        elif kind == "tile_first":                            # first key of a 32 / 64 / 128-key tile
            take("fire", lambda i: k_a, before=True)
        elif kind == "tile_last":                             # last key of one
            take("fire", lambda i: k_a + 127 if k_a + 127 < sk - 1 else k_a - 1, before=True)
        elif kind == "last_key":                              # Sk - 1, inside the partial last tile: the factor is still pending in the epilogue
            # (where the 20 % rule cannot hold at Sk - 1 -- at thr = 0 a +2 spike is outweighed by the keys ahead of it -- the placement stays, as a `tail`: the rule is
            # not needed to see a factor dropped in the epilogue, which multiplies everything ahead of the spike by 2^(thr + 2))
            take("fire", lambda i: sk - 1, before=True) or take("tail", lambda i: sk - 1 if hi[i] == sk - 1 and sk - 1 - lo[i] >= 40 else None)
        elif kind == "diag" and wr >= 0:                      # the row's last visible key, a decoy just past it in the same step
            take("fire", lambda i: int(hi[i]) if hi[i] < sk - 1 else None, decoy_of=lambda i: int(hi[i]) + 1, before=True)
        elif kind == "win_lo" and wl >= 0:                    # the first visible key of a window, a decoy just left of it in the same step
            take("fire", lambda i: int(lo[i]) if lo[i] > 0 and hi[i] - lo[i] >= 40 else None, decoy_of=lambda i: int(lo[i]) - 1)
        elif kind == "hold":
            take("hold", lambda i: int(lo[i]) + (min(sk, int(hi[i]) + 1) - int(lo[i])) // 2 if hi[i] - lo[i] >= 40 else None)
        elif kind == "twice":
            take("twice", lambda i: (96 if thr <= 2 else k_a + 32) if k_a + 64 < sk else None, span=2, before=True)   # (thr = 0: a +2 spike needs FEW keys ahead)
        elif kind == "stairs":
            take("stairs", lambda i: min(k_a + 64, sk - 100) if sk >= 140 else None, span=4)
        elif kind == "split_first" and edges:                 # first key of the last split that holds keys: the other splits hold background only
            take("fire", lambda i: max([e for e in edges if e <= hi[i]] or [None]), before=True)
        elif kind == "split_last" and edges:                  # last key of the split before it
            take("hold", lambda i: max([e for e in edges if 0 < e <= hi[i]] or [0]) - 1 if [e for e in edges if 0 < e <= hi[i]] else None)
        elif kind == "past_len":                              # a fire at the last key, a decoy behind the entry's length (the caller's cache holds it)
            take("fire", lambda i: sk - 1 if hi[i] == sk - 1 else None, decoy_of=lambda i: sk, before=True, past=True)
    return plan


def placements_of(plan):
    return sorted({kind + ("+decoy" if dk is not None else "") + ("@%d" % (keys[0] % 128)) for kind, _, _, keys, dk in plan})


# ---------------------------------------------------------------- the builder ----------------------------------------------------------------
class Profile:
    """One batch entry: q (Sq, H, D), k (Sk + extra, Hk, D), v (Sk + extra, Hk, Dv) fp32 holding values of the input dtype; `extra` rows behind Sk carry the decoys past the
    entry's length.  s2 (H, Sq, Sk) fp64: the scores in log2 units, -inf where masked.  targets: [(kind, row, head, key, height)], decoys included."""


def _round(t, dtype):
    return t.to(dtype).to(torch.float32)


def _scores2(q, k, sq, sk, mask, softcap, slopes):
    """fp64 scores of the finished tensors in log2 units, UNMASKED (H, Sq, Sk), and the visible set (Sq, Sk)."""
    h, g = q.shape[1], q.shape[1] // k.shape[1]
    raw = torch.einsum("ihd,jhd->hij", q.double(), k[:sk].double().repeat_interleave(g, 1)) * SCALE
    if softcap > 0:
        raw = softcap * torch.tanh(raw / softcap)
    if slopes is not None:
        i = torch.arange(sq, dtype=torch.float64)[:, None] + (sk - sq)
        j = torch.arange(sk, dtype=torch.float64)[None, :]
        raw = raw - torch.as_tensor(slopes, dtype=torch.float64)[:, None, None] * (i - j).abs()[None]
    wl, wr = window_of(sq, sk, mask, slopes is not None)
    return raw * LOG2E, torch.from_numpy(orc.visible_mask(sq, sk, wl, wr))


def build(dtype, d, dv, sq, sk, h, hk, mask, thr, plan, seed=0, softcap=0.0, slopes=None, c0=0, extra=0, codes=True, v_is_k=False, targets=True):
    """-> Profile.  dtype: a key of DT.  plan: make_plan()'s list.  targets=False: the same tensors with the targets removed (the background alone).
    softcap: a capped score cannot exceed softcap * log2(e) log2 units -- the heights must stay under it (asserted).  c0: first target channel (MLA: 512, the rope part,
    so that V = K[..., :512] stays clean; v_is_k makes V that view).  slopes: ALiBi slopes per head (the bias is part of the height)."""
    tdt = DT[dtype]
    g = torch.Generator().manual_seed(1000 + seed)
    n_t = sum(len(keys) + (dk is not None) for _, _, _, keys, dk in plan)
    assert c0 + n_t <= d, "not enough channels for %d targets" % n_t
    bgc = [c for c in range(d) if not c0 <= c < c0 + n_t and not (v_is_k and c < 4)]   # (MLA: the coded columns of V are channels of K -- q is zero there)
    sig_k = 1.0 if v_is_k else math.sqrt(BG / (C * math.sqrt(len(bgc))))
    sig_q = BG / (C * math.sqrt(len(bgc))) / sig_k
    q, k = torch.zeros(sq, h, d), torch.zeros(sk + extra, hk, d)
    q[..., bgc] = torch.randn(sq, h, len(bgc), generator=g) * sig_q
    k[..., bgc] = torch.randn(sk + extra, hk, len(bgc), generator=g) * sig_k
    v = k if v_is_k else torch.randn(sk + extra, hk, dv, generator=g)   # (MLA: the codes below are written into K's first channels, which ARE V)
    if codes or v_is_k:
        j = torch.arange(sk + extra)
        v[:, :, 0] = (4.0 - 8.0 * ((j // 64) % 2))[:, None]
        v[:, :, 1] = (4.0 - 8.0 * (j >= sk // 2).float())[:, None]
        v[:, :, 2] = (4.0 - 8.0 * ((j // STEP) % 2))[:, None]
        v[:, :, 3] = (4.0 - 8.0 * (j >= max(128, (int(0.72 * sk) // 128) * 128)).float())[:, None]   # (the keys ahead of make_plan's tile-aligned fires)
    q, k = _round(q, tdt), _round(k, tdt)
    v = k[..., :dv] if v_is_k else _round(v, tdt)
    lo, hi = bounds(sq, sk, mask, slopes is not None)
    grp = h // hk
    s_bg, vis = _scores2(q, k, sq, sk, mask, 0.0, None)        # (the background's RAW scores: softcap and the bias are inverted below)
    cap2 = softcap * LOG2E
    out_t, ch = [], c0
    for kind, row, head, keys, dk in plan:
        run = s_bg[head, row].clone()                            # the row's final scores so far, unmasked
        if softcap > 0:
            run = cap2 * torch.tanh(run / cap2)
        bias = torch.zeros(sk, dtype=torch.float64)
        if slopes is not None:
            bias = -float(slopes[head]) * LOG2E * (row + sk - sq - torch.arange(sk, dtype=torch.float64)).abs()
            run = run + bias
        first = float(run[lo[row]])
        base = None
        fire_h = None
        for n, key in enumerate(keys):
            prior = float(run[lo[row]:key].max()) if key > lo[row] else None
            if kind in ("fire", "twice", "tail"):
                height = FIRST_HEIGHT if prior is None else prior + thr + 2
                fire_h = height
            elif kind == "hold":
                height = first + thr - 1
            else:
                base = prior if base is None else base
                height = base + 6 * (n + 1)
            out_t.append((kind, row, head, key, height, ch))
            run[key] = height
            ch += 1
        if dk is not None:
            out_t.append(("decoy", row, head, dk, fire_h + 3, ch))
            ch += 1
    if targets:
        for kind, row, head, key, height, c in out_t:
            want = height - (float(bias_of(slopes, head, row, key, sq, sk)) if slopes is not None else 0.0)
            if softcap > 0:
                assert abs(want) < cap2 - 0.05, "height %.2f does not fit under the cap of %.2f log2 units" % (want, cap2)
                want = cap2 * math.atanh(want / cap2)
            q[row, head, c] = 1.0
            kval = (want - float(s_bg[head, row, key] if key < sk else 0.0)) / C
            k[key, head // grp, c] = kval
        k = _round(k, tdt)
        if v_is_k:
            v = k[..., :dv]
    p = Profile()
    p.dtype, p.d, p.dv, p.sq, p.sk, p.h, p.hk, p.mask, p.thr, p.softcap, p.slopes, p.extra = dtype, d, dv, sq, sk, h, hk, tuple(mask), thr, softcap, slopes, extra
    p.q, p.k, p.v, p.vis, p.plan = q, k, v, vis, plan
    p.targets = [t[:5] for t in out_t] if targets else []
    s2, _ = _scores2(q, k, sq, sk, mask, softcap, slopes)
    p.s2_open = s2                                               # unmasked (mutant "mask_lost" reads it)
    p.s2 = s2.masked_fill(~vis[None], float("-inf"))
    if extra and targets:                                        # the decoys behind the entry's length: scored as if they were visible
        p.past = [(row, head, key, float((q[row, head].double() @ k[key, head // grp].double()) * C)) for kind, row, head, key, _ in p.targets if kind == "decoy" and key >= sk]
    return p


def bias_of(slopes, head, row, key, sq, sk):
    return -float(slopes[head]) * LOG2E * abs(row + sk - sq - key)


def check_conditions(p):
    """The builder's conditions on the fp64 scores of the finished tensors (the module docstring).  -> {(row, head, key): the smaller of the two masses} of the fires
    that carry the 20 % rule."""
    lo, hi = bounds(p.sq, p.sk, p.mask, p.slopes is not None)
    masses, pair = {}, {}
    for kind, row, head, key, height in p.targets:
        s = p.s2[head, row]
        top = float(s[torch.isfinite(s)].max())
        if kind == "decoy":
            assert key >= p.sk or not bool(p.vis[row, key]), ("a decoy is visible", row, head, key)
            open_s = float(p.s2_open[head, row, key]) if key < p.sk else [x[3] for x in p.past if x[:3] == (row, head, key)][0]
            assert open_s > top + 2, ("a decoy would not show", row, head, key, open_s, top)
            continue
        # (e4m3 holds k = height / 0.1875 to 1 part in 16: the height IS what the tensor holds -- within 0.45 of the plan up to 12 units, coarser above, where only stairs go)
        slack = 0.1 if p.dtype != "e4m3" else (0.45 if height < 12 else 1.6)
        assert bool(p.vis[row, key]) and abs(float(s[key]) - height) < slack, (kind, row, head, key, float(s[key]), height)
        first = float(s[lo[row]])
        prior = float(s[lo[row]:key].max()) if key > lo[row] else None
        w = torch.exp2(s - top)
        if kind == "hold":
            assert float(s[key]) <= first + p.thr - 0.5, ("hold", row, head, float(s[key]) - first)
        if kind not in ("fire", "twice", "tail") or prior is None:
            continue
        assert float(s[key]) >= prior + p.thr + 0.5, (kind, row, head, float(s[key]) - prior)
        if p.thr > 8 or kind == "tail":
            continue
        if kind == "twice" and (row, head) not in pair:          # the first growth of the pair, judged on the keys ahead of the second one
            pair[(row, head)] = float(w[:key].sum()) * 2.0 ** (float(s[key]) - prior)
            w = w[:key + STEP]
        elif kind == "twice" and p.thr > 2:                      # the second: what a LOST first factor would leave in the row
            assert pair[(row, head)] / float(w.sum()) >= 0.2, ("twice: a lost first factor would not show", row, head, pair[(row, head)] / float(w.sum()))
            continue
        before, after = float(w[:key].sum()) / float(w.sum()), float(w[key:].sum()) / float(w.sum())
        assert min(before, after) >= 0.2, (kind, row, head, key, before, after)
        masses[(row, head, key)] = min(before, after)
    return masses


# ---------------------------------------------------------------- references ----------------------------------------------------------------
def oracle(p):
    """The fp64 oracle on the profile's tensors -> out (Sq, H, Dv), lse (H, Sq) numpy.  (attention_fwd has one head dim: V is zero-padded to D.)"""
    v = p.v[:p.sk]
    if p.dv != p.d:
        v = torch.cat([v, torch.zeros(p.sk, p.hk, p.d - p.dv)], -1)
    sl = None if p.slopes is None else np.asarray(p.slopes, dtype=np.float64)
    o, l = orc.attention_fwd(p.q[None], p.k[None, :p.sk], v[None], SCALE, bool(p.mask[0]), (p.mask[1], p.mask[2]), p.softcap, sl)
    return o[0][..., :p.dv], l[0]


def baseline(p, device="cpu", dout=None):
    """Plain PyTorch attention computing in the input dtype (the yardstick of the 2x / 3x rule; tools/fuzz_gpu.py torch_baseline with an explicit scale) -> out fp32,
    and with dout (Sq, H, Dv) also dq, dk, dv through autograd."""
    dt = DT[p.dtype] if p.dtype != "e4m3" else torch.bfloat16
    q, k, v = (t.to(device=device, dtype=dt).requires_grad_(dout is not None) for t in (p.q, p.k[:p.sk], p.v[:p.sk]))
    g = p.h // p.hk
    kk, vv = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    s = torch.einsum("ihd,jhd->hij", q * SCALE, kk)
    if p.softcap > 0:
        s = p.softcap * torch.tanh(s / p.softcap)
    i = torch.arange(p.sq, device=device)[:, None] + (p.sk - p.sq)
    j = torch.arange(p.sk, device=device)[None, :]
    if p.slopes is not None:
        s = s + (-(i - j).abs().to(s.dtype))[None] * torch.as_tensor(p.slopes, device=device).to(s.dtype)[:, None, None]
    vis = p.vis.to(device)
    s = s.masked_fill(~vis[None], float("-inf"))
    pr = torch.softmax(s, dim=-1).masked_fill(~vis.any(-1)[None, :, None], 0.0)
    out = torch.einsum("hij,jhc->ihc", pr, vv)
    if dout is None:
        return out.float().cpu()
    return (out.detach().float().cpu(),) + tuple(t.float().cpu() for t in torch.autograd.grad(out, (q, k, v), dout.to(device=device, dtype=dt)))


SPEC_DEFAULTS = dict(dv=None, h=2, hk=1, mask=(False, -1, -1), thr=8, seed=0, softcap=0.0, slopes=None, c0=0, extra=0, codes=True, v_is_k=False, edges=(),
                     kinds=("first", "tile_first", "tile_last", "last_key", "diag", "win_lo", "hold", "twice", "stairs"))


def spec(dtype, d, sq, sk, **kw):
    """A case's inputs as a hashable spec: the fields of SPEC_DEFAULTS over (dtype, d, sq, sk)."""
    s = dict(SPEC_DEFAULTS, dtype=dtype, d=d, sq=sq, sk=sk, **kw)
    s["dv"] = s["dv"] or d
    return tuple(sorted(s.items()))


@functools.lru_cache(maxsize=None)
def profile_of(sp, targets=True):
    s = dict(sp)
    plan = make_plan(s["sq"], s["sk"], s["mask"], s["thr"], s["h"], s["edges"], s["kinds"], s["slopes"] is not None, 0.4 if s["dtype"] == "e4m3" else 0.0)
    p = build(s["dtype"], s["d"], s["dv"], s["sq"], s["sk"], s["h"], s["hk"], s["mask"], s["thr"], plan, s["seed"], s["softcap"], s["slopes"], s["c0"], s["extra"],
              s["codes"], s["v_is_k"], targets)
    p.masses = check_conditions(p)
    return p


@functools.lru_cache(maxsize=None)
def reference(sp):
    """-> (profile, oracle out (Sq, H, Dv) fp64, oracle lse (H, Sq) fp64, the same-dtype PyTorch error): computed once, shared, never modified."""
    p = profile_of(sp)
    o, l = oracle(p)
    o, l = torch.from_numpy(o), torch.from_numpy(l)
    return p, o, l, float((baseline(p).double() - o).abs().max())


# ---------------------------------------------------------------- the stand-in ----------------------------------------------------------------
def standin(p, thr, mutant=None, step=STEP):
    """The deferred, lagged online softmax on the profile's tensors -> out (Sq, H, Dv) fp32 holding values of the output dtype, lse (H, Sq) fp32 (natural log).
    mutant: one of MUTANTS, the mistake a kernel could make."""
    assert mutant is None or mutant in MUTANTS
    fp8 = p.dtype == "e4m3"
    pdt = DT[p.dtype]
    odt = torch.bfloat16 if fp8 else pdt
    g = p.h // p.hk
    # Q' = q * scale * log2(e), rounded once (exact for e4m3 inputs: the kernel scales the fp32 scores); under softcap the multiplier is 2 scale log2(e) / softcap
    # (fa_fwd_w64.hip: the chains deliver 2 log2(e) score / softcap), which is exact only for a softcap like SOFTCAP
    cq = 2 * C / p.softcap if p.softcap > 0 else C
    qs = p.q * cq if fp8 else _round(p.q * cq, pdt)
    kf, vf = p.k[:p.sk].repeat_interleave(g, 1), p.v[:p.sk].repeat_interleave(g, 1)
    s_open = torch.einsum("ihd,jhd->hij", qs, kf)                # (H, Sq, Sk) fp32, log2 units
    if p.softcap > 0:
        s_open = (p.softcap * LOG2E) * torch.tanh(s_open / (2 * LOG2E))
    if p.slopes is not None:
        i = torch.arange(p.sq, dtype=torch.float32)[:, None] + (p.sk - p.sq)
        j = torch.arange(p.sk, dtype=torch.float32)[None, :]
        s_open = s_open - (torch.as_tensor(p.slopes, dtype=torch.float32) * LOG2E)[:, None, None] * (i - j).abs()[None]
    s_all = s_open.masked_fill(~p.vis[None], float("-inf"))
    h, sq, sk = s_all.shape
    ninf = float("-inf")
    m = torch.full((h, sq), ninf)
    thr_l = torch.full((h, sq), thr if mutant == "first_no_grow" else ninf)
    l = torch.zeros(h, sq)
    o = torch.zeros(h, sq, p.dv)
    pending = torch.ones(h, sq)
    prev_t = torch.full((h, sq), ninf)
    p_prev, v_prev = None, None
    vh = vf.permute(1, 0, 2)                                     # (H, Sk, Dv)
    pad = (-sq) % 32

    def group_min(x):                                            # the smallest factor of each 32-row group, handed to all its rows
        xp = torch.cat([x, torch.ones(h, pad)], 1).reshape(h, -1, 32)
        return xp.min(-1, keepdim=True).values.expand(-1, -1, 32).reshape(h, -1)[:, :sq]

    for t0 in range(0, sk, step):
        s = s_all[:, :, t0:t0 + step]
        tmax = s.max(-1).values
        m_base = torch.where(m == ninf, torch.zeros(()), m)
        if mutant == "prev_tile":                                # the threshold against the previous tile's maximum instead of m
            ref = torch.where(prev_t == ninf, torch.full((), ninf), prev_t)
            grow = torch.where(m == ninf, tmax > ninf, (tmax - ref) > thr)
            grow &= tmax > m
            prev_t = torch.where(tmax > ninf, tmax, prev_t)
        else:
            grow = (tmax - m_base) > thr_l
        m_new = torch.where(grow, tmax, m)
        m_safe = torch.where(m_new == ninf, torch.zeros(()), m_new)
        alpha = torch.where(grow & (m != ninf), torch.exp2(m - m_safe), torch.ones(()))
        thr_l = torch.where(grow, torch.full((), float(thr)), thr_l)
        m = m_new
        if mutant != "l_not":
            l = l * alpha
        # the factor of the previous decision reaches O now, one step late
        f = pending
        if mutant == "group_factor":
            f = group_min(pending)
        if mutant == "overwrite":                                # a growth in the very next step overwrites the factor that was waiting
            f = torch.where(grow & (alpha != 1), torch.ones(()), f)
        if mutant == "o_never":
            f = torch.ones(h, sq)
        o = o * f[..., None]
        if mutant == "o_twice":
            o = o * f[..., None]
        pending = alpha
        if p_prev is not None:
            o = o + torch.einsum("hij,hjc->hic", p_prev, v_prev)
        if mutant == "mask_lost":                                # the growing step's mask is rewritten away
            s = torch.where((grow & (alpha != 1))[..., None], s_open[:, :, t0:t0 + step], s)
        pr = torch.exp2(s - m_safe[..., None])
        l = l + pr.sum(-1)
        p_prev, v_prev = _round(pr, pdt), vh[:, t0:t0 + step]
    f = group_min(pending) if mutant == "group_factor" else pending
    if mutant not in ("epilogue_drop", "o_never"):
        o = o * f[..., None]
        if mutant == "o_twice":
            o = o * f[..., None]
    if p_prev is not None:
        o = o + torch.einsum("hij,hjc->hic", p_prev, v_prev)
    live = m != ninf
    l_safe = torch.where(live & (l > 0), l, torch.ones(()))
    out = torch.where(live[..., None], o / l_safe[..., None], torch.zeros(()))
    lse = torch.where(live, (m + torch.log2(l_safe)) / LOG2E, torch.full((), float("inf")))
    return _round(out.permute(1, 0, 2), odt), lse


# ---------------------------------------------------------------- judging ----------------------------------------------------------------
def judge(out, lse, o_ref, l_ref, out_tol, lse_tol=LSE_BOUND):
    """out (Sq, H, Dv) / lse (H, Sq) against the oracle's -> (out error / tolerance, lse error / tolerance, problems: list of str).  out_tol: a number or a tensor like
    out (element by element).  A NaN or an inf in out, an LSE that is not +inf exactly where the oracle's is, count as problems whatever the figures say."""
    o, l = out.detach().double().cpu(), lse.detach().double().cpu()
    problems = []
    if not bool(torch.isfinite(o).all()):
        problems.append("out holds %d non-finite elements" % int((~torch.isfinite(o)).sum()))
    fin = torch.isfinite(l_ref)
    if not torch.equal(torch.isposinf(l), ~fin):
        problems.append("LSE is not +inf exactly on the rows that see no key")
    err = torch.nan_to_num((o - o_ref).abs(), nan=float("inf"), posinf=float("inf"))
    r_o = float((err / out_tol).max())
    both = fin & torch.isfinite(l)
    tol_l = lse_tol if lse_tol is not None else 5e-4 * l_ref[both].abs().clamp(min=1.0)   # (None: the relative rule of the e4m3 families)
    r_l = float(((l[both] - l_ref[both]).abs() / tol_l).max()) if bool(both.any()) else 0.0
    if not r_o <= 1.0:
        problems.append("out error %.3e, %.2f x its tolerance" % (float(err.max()), r_o))
    if not r_l < 1.0:
        problems.append("lse error %.2f x its tolerance" % r_l)
    return r_o, r_l, problems


# ---------------------------------------------------------------- the case lists of tests/test_softmax_profiles_gpu.py ----------------------------------------------------------------
BIG, SMALL = (600, 1100), (160, 333)       # default threshold / FA_RESCALE_THR=0 (the 20 % condition sizes both)
MASKS = {BIG: [(False, -1, -1), (True, -1, -1), (False, 700, 60)], SMALL: [(False, -1, -1), (True, -1, -1), (False, 100, 20)]}
CACHE_CAP, CACHE_LENS = 1536, (1100, 300)   # 24 tiles of 64 keys: splits of 12 / 8 / 6 tiles (first keys 768 / 1024 / 768 of the last one that holds keys); the short entry leaves the later splits empty
CACHE_LENS_SMALL = (333, 100)
DECODE_KINDS = ("split_first", "split_last", "past_len", "twice", "first", "hold", "stairs")
SLOPES = (0.001, 0.002)


def split_edges(splits, cap=CACHE_CAP):
    """First keys of the KV splits fa_api.cpp choose_splits makes of a cache of `cap` rows (whole 64-key tiles, ceil(tiles / splits) each)."""
    tiles = -(-cap // 64)
    per = -(-tiles // max(splits, 1))
    return tuple(range(0, cap, per * 64)) if splits > 1 else (768,)


def fwd_list(dtype, d, thr, dv=None, masks=None, **kw):
    shape = SMALL if thr == 0 else BIG
    return [spec(dtype, d, shape[0], shape[1], mask=m, thr=thr, dv=dv, **kw) for m in (masks or MASKS[shape])]


def cache_list(dtype, d, sq, splits, thr=8, **kw):
    """The entries of one KV-cache batch: cache_seqlens = CACHE_LENS (thr = 0: CACHE_LENS_SMALL), causal where Sq > 1, one row behind each entry's length for the decoy."""
    h, hk = kw.pop("h", 4), kw.pop("hk", 2)
    return [spec(dtype, d, sq, n, h=h, hk=hk, mask=(sq > 1, -1, -1), thr=thr, seed=b, extra=1, edges=split_edges(splits) if thr else (128,), kinds=DECODE_KINDS, **kw)
            for b, n in enumerate(CACHE_LENS if thr else CACHE_LENS_SMALL)]


def mla_list(dtype, sq, splits):
    return cache_list(dtype, 576, sq, splits, dv=512, h=16, hk=1, c0=512, v_is_k=True)


@functools.lru_cache(maxsize=None)
def case_lists():
    """{list name: [spec]}: every set of inputs the GPU module runs, by kernel family.  The CPU module runs the stand-in and its mutants over the same lists."""
    out = {}
    for dt in ("bf16", "fp16"):
        for d in (64, 128):
            out["fwd %s d%d thr8" % (dt, d)] = fwd_list(dt, d, 8)
            out["fwd %s d%d thr0" % (dt, d)] = fwd_list(dt, d, 0)
        out["fwd fp16 thr15"] = [s for d in (64, 128) for s in fwd_list("fp16", d, 15, masks=[(True, -1, -1)])]
        out["lockstep dims %s" % dt] = [s for d in (256, 96, 40) for s in fwd_list(dt, d, 8, masks=MASKS[BIG][:2])]
        out["packed gqa %s" % dt] = [spec(dt, 128, 16, 1100, h=4, hk=1, mask=m, thr=8, kinds=("tile_first", "tile_last", "last_key", "hold", "twice", "stairs", "first"))
                                      for m in MASKS[BIG][:2]]
        out["w64 alibi %s" % dt] = [spec(dt, d, 600, 1100, mask=(True, -1, -1), thr=8, slopes=SLOPES) for d in (64, 128)]
        out["w64 softcap %s" % dt] = [spec(dt, d, 600, 1100, mask=m, thr=8, softcap=SOFTCAP) for d, m in ((64, MASKS[BIG][1]), (128, MASKS[BIG][2]))]
        # (512 rows = 2 blocks of 256 per head: under a right-bounded mask the persistent walk needs rounds made of whole units, 32 % (blocks per unit) == 0)
        out["w64 persist %s" % dt] = [spec(dt, d, 512, 1100, mask=m, thr=8) for d, m in ((128, MASKS[BIG][1]), (128, MASKS[BIG][0]), (64, MASKS[BIG][1]))]
        out["dv %s" % dt] = fwd_list(dt, 192, 8, dv=128) + fwd_list(dt, 192, 0, dv=128)
        for sq in (1, 2):
            for splits in (1, 3):
                out["mla %s sq%d splits%d" % (dt, sq, splits)] = mla_list(dt, sq, splits)
        for sq in (1, 4):
            for splits in (1, 2, 3, 4):
                out["kvcache %s sq%d splits%d" % (dt, sq, splits)] = cache_list(dt, 128, sq, splits)
    for d in (64, 128):
        out["fp8 d%d thr8" % d] = fwd_list("e4m3", d, 8)
        out["fp8 d%d thr0" % d] = fwd_list("e4m3", d, 0)
    for sq in (1, 4):
        out["fp8 kvcache sq%d" % sq] = cache_list("e4m3", 128, sq, 1)
        out["fp8 kvcache sq%d thr0" % sq] = cache_list("e4m3", 128, sq, 1, thr=0)
    return out


def live(mutant, p):
    """Can the mutant show on this profile?  (From the plan alone: what the placement was made for.)"""
    fires = [t for t in p.targets if t[0] in ("fire", "twice", "tail") and t[3] > bounds(p.sq, p.sk, p.mask, p.slopes is not None)[0][t[1]]]
    if mutant in ("o_twice", "overwrite", "group_factor") and p.dtype == "e4m3" and p.thr > 2:
        # the e4m3 families are judged against an emulation that rounds the NORMALISED P to e4m3 (tests/test_fwd_fp8_gpu.py _emulate): it drops every key below 2^-10 of
        # its row, i.e. the whole background of a row with the ~550 keys the 20 % condition needs at thr = 8, and the tolerance is twice that loss.  A factor applied
        # twice moves the row by less; the thr = 0 lists (333 keys) carry these three mutants for the e4m3 kernels.  
        return False
    if mutant in ("o_never", "o_twice", "l_not"):
        return bool(p.masses)
    if mutant == "group_factor":
        return bool(p.masses) and p.sq >= 32
    if mutant == "epilogue_drop":
        return any(t[3] // STEP == (p.sk - 1) // STEP for t in fires) and p.thr <= 8
    if mutant == "overwrite":
        return any(t[0] == "twice" for t in p.targets) and p.thr <= 8
    if mutant == "mask_lost":
        return any(t[0] == "decoy" and t[3] < p.sk for t in p.targets)
    if mutant == "prev_tile":
        return p.dtype == "fp16" and p.thr >= 6 and any(t[0] == "stairs" for t in p.targets)
    if mutant == "first_no_grow":
        return p.thr >= 1
    raise KeyError(mutant)


def family_of(name):
    """The kernel family of a list name, which decides the rule its cases are judged by."""
    for fam in ("fp8 kvcache", "fp8", "kvcache", "mla", "dv"):
        if name.startswith(fam):
            return fam
    return "fwd"


def out_tolerance(family, p, o_ref, err_pt):
    """The out rule the family already has (none is changed here):
      fwd      tools/fuzz_gpu.py, the reference's rule: 2 x the same-dtype PyTorch error + 1e-5
      dv, mla  tests/test_headdim_v_gpu.py / tests/test_mla_decode_gpu.py _check: 2 x the same-dtype PyTorch error + 1e-4
      kvcache  tests/test_kvcache_gpu.py: 2e-2 absolute on a bf16 out, 5e-3 on an fp16 one
      fp8 ..   tests/test_fwd_fp8_gpu.py _check_parity / tests/test_kvcache_fp8_gpu.py _check_entry: 2 max|emu - ref| + 2 bf16-eps |ref| + 1e-6, element by element
               (the GPU module calls those functions themselves; this is their arithmetic for the stand-in)."""
    if family == "fwd":
        return 2 * err_pt + 1e-5
    if family in ("dv", "mla"):
        return 2 * err_pt + 1e-4
    if family == "kvcache":
        return 2e-2 if p.dtype == "bf16" else 5e-3
    from tests.test_fwd_fp8_gpu import BF16_EPS, _emulate
    emu = torch.from_numpy(_emulate(p.q[None].double().numpy(), p.k[None, :p.sk].double().numpy(), p.v[None, :p.sk].double().numpy(), SCALE, bool(p.mask[0]), p.mask[1:]))[0]
    return 2 * float((emu - o_ref).abs().max()) + 2 * BF16_EPS * o_ref.abs() + 1e-6
