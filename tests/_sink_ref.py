"""Learnable attention sinks: the float64 formulas of the post-pass, a torch stand-in with the kernels' roundings, the fixture's loader and the reference's two
acceptance rules, restated (test infrastructure only).

    lse' = log(exp(lse) + exp(s)),  out' = out / (1 + exp(s - lse)),  dsink[h] = - sum_rows exp(s_h - lse') * softmax_d,  softmax_d = rowsum(dout * out')

A row whose lse is not finite has no visible key: out' = 0, lse' = s, lse_bwd = +inf, and it is left out of the dsink sum.  A sink of -inf is the identity (a row
without a key keeps its marker then)."""
import glob
import math
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LSE_TOL = 2e-3                # the bound of tests/test_golden_matrix_gpu.py for lse under the default knobs
QUANTITIES = ("out", "dq", "dk", "dv", "dsink")
STANDIN_VARIANTS = (0, 1, 2)
DSINK_VARIANTS = tuple(range(16))
MISTAKES = ("lse_without_sink", "dsink_sign", "sink_per_kv_head", "empty_lse_inf", "empty_rows_in_dsink")


# ---- float64 formulas ------------------------------------------------------------------------------------------------------------------------------------
def _np64(x):
    return x.detach().double().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


def apply_ref64(out, lse, sink):
    """out (.., S, H, D) with lse (.., H, S) -- (B, S, H, D) / (B, H, S) or (total, H, D) / (H, total) --, sink (H) -> float64 (out', lse', lse_bwd).
    Rows without a key (lse not finite) are not multiplied: NaN there does not reach the reference either."""
    out, lse, sink = _np64(out), _np64(lse), _np64(sink)
    s = np.broadcast_to(sink[:, None], lse.shape)
    live = np.isfinite(lse)
    off = np.isneginf(s)
    with np.errstate(over="ignore", invalid="ignore"):
        l0 = np.where(live, lse, 0.0)
        f = np.where(live, np.where(off, 1.0, 1.0 / (1.0 + np.exp(np.where(off, 0.0, s) - l0))), 0.0)
        lse2 = np.where(off, lse, np.where(live, np.maximum(l0, s) + np.log1p(np.exp(-np.abs(l0 - np.where(off, 0.0, s)))), s))
    lse_bwd = np.where(live, lse2, np.inf)
    fo = np.swapaxes(f, -1, -2)[..., None]
    return np.where(fo > 0, out, 0.0) * fo, lse2, lse_bwd


def dsink_ref64(softmax_d, lse_bwd, sink):
    """softmax_d, lse_bwd (.., H, S), sink (H) -> (dsink (H) float64, sum of |terms| (H)): rows with a non-finite lse_bwd are skipped, their softmax_d unread."""
    d, l, sink = _np64(softmax_d), _np64(lse_bwd), _np64(sink)
    live = np.isfinite(l)
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.where(live, np.exp(sink[:, None] - np.where(live, l, 0.0)), 0.0)
    terms = np.where(w > 0, np.where(w > 0, d, 0.0) * w, 0.0)
    axes = tuple(i for i in range(terms.ndim) if i != terms.ndim - 2)
    return -terms.sum(axes), np.abs(terms).sum(axes)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------------------
def fixture_files():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "sink_ref_cases*.npz")))


_CASES = None


def load_cases():
    """{case name: {key: array}} of tests/golden/sink_ref_cases*.npz (tests/golden/make_sink_golden.py)."""
    global _CASES
    if _CASES is None:
        cases = {}
        for path in fixture_files():
            with np.load(path) as z:
                for k in z.files:
                    if "/" in k:
                        cases.setdefault(k.split("/")[0], {})[k.split("/", 1)[1]] = z[k]
        _CASES = cases
    return _CASES


def case_meta(case):
    H, Hk, D, causal, wl, wr = (int(x) for x in case["meta"])
    return dict(H=H, Hk=Hk, D=D, causal=bool(causal), window=(wl, wr), softcap=float(case["softcap"][0]), packed=int(case["packed"][0]) == 1,
                qlens=[int(x) for x in case["qlens"]], klens=[int(x) for x in case["klens"]])


def case_inputs(case, dtype, device=None):
    """q, k, v, do (every value exact in bf16 and in fp16) and the fp32 sink (exact in both as well).  A packed case: (total, H, D); else (B, S, H, D)."""
    ts = [torch.from_numpy((case[nm + "_bf16bits"].astype(np.uint32) << 16).view(np.float32).copy()).to(dtype) for nm in ("q", "k", "v", "do")]
    ts.append(torch.from_numpy(case["sink"].copy()))
    return [t if device is None else t.to(device) for t in ts]


def sequences(case):
    """[(q slice, k slice)] per sequence, on the leading dimension of the stored tensors viewed as (total, H, D) (a fixed-length case is viewed flat)."""
    m = case_meta(case)
    cq, ck = np.concatenate([[0], np.cumsum(m["qlens"])]), np.concatenate([[0], np.cumsum(m["klens"])])
    return [(slice(int(cq[i]), int(cq[i + 1])), slice(int(ck[i]), int(ck[i + 1]))) for i in range(len(m["qlens"]))]


# ---- the stand-in ---------------------------------------------------------------------------------------------------------------------------------------
def visible(sq, sk, causal, window):
    """(sq, sk) bool: this package's masks, aligned to the bottom-right corner."""
    i, j = torch.arange(sq)[:, None], torch.arange(sk)[None, :]
    wl, wr = window
    if causal:
        wr = 0
    vis = torch.ones(sq, sk, dtype=torch.bool)
    if wr >= 0:
        vis &= j <= i + sk - sq + wr
    if wl >= 0:
        vis &= j >= i + sk - sq - wl
    return vis


def standin(case, dtype, mistake=None, variant=0):
    """What the kernels compute, in torch on the CPU with their roundings: attention in fp32 with the probabilities rounded to `dtype` in front of the product
    with V (as the forward kernels feed their matrix instructions), out rounded to `dtype`, the sink factor applied in fp32 and out' rounded again, then the
    FA-2 backward formulas on (out', lse_bwd) with P and dS rounded to `dtype`, softmax_d = rowsum(dout * out') poisoned with NaN on rows without a key (a
    backward schedule may leave it unwritten there), and dsink from softmax_d.  `mistake`: one of MISTAKES, built in on purpose.  `variant`: which realisation of the
    forward's rounding noise (below); the allowance of a case is 2 x ONE realisation of the reference's own error, so the fixture is held to half of it on all of
    STANDIN_VARIANTS.  out, dq, dk and dv are judged by the worst of thousands of elements, which one realisation samples well.  dsink is H sums of that noise
    over a whole head each, one draw per head and realisation, so it is held to half of its allowance on all sixteen DSINK_VARIANTS: noise that passes sixteen
    draws at 0.5 has a standard deviation near a quarter of the allowance at the most, which puts the rule itself four of them away for any other
    realisation -- the GPU's.
    -> {out, lse, dq, dk, dv (the case's layout, fp32), dsink (H) fp32}."""
    assert mistake is None or mistake in MISTAKES, mistake
    m = case_meta(case)
    q, k, v, do, sink = case_inputs(case, dtype)
    H, Hk, D = m["H"], m["Hk"], m["D"]
    g = H // Hk
    shape_q, shape_k = q.shape, k.shape
    q, k, v, do = (t.reshape(-1, t.shape[-2], D).float() for t in (q, k, v, do))
    s_head = sink.repeat_interleave(g)[:H] if mistake == "sink_per_kv_head" else sink          # (sink[h // g]: the first Hk entries, each g times)
    out_all, lse_all = torch.zeros_like(q), torch.zeros(H, q.shape[0])
    dq_all, dk_all, dv_all, dsink = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v), torch.zeros(H, dtype=torch.float64)
    for sq_, sk_ in sequences(case):
        qs, ks, vs, dos = q[sq_], k[sk_].repeat_interleave(g, 1), v[sk_].repeat_interleave(g, 1), do[sq_]
        Sq, Sk = qs.shape[0], ks.shape[0]
        if Sq == 0:
            continue
        S = torch.einsum("thd,shd->hts", qs, ks) / math.sqrt(D)
        if m["softcap"] > 0:
            S = torch.tanh(S / m["softcap"]) * m["softcap"]
        vis = visible(Sq, Sk, m["causal"], m["window"])
        S = S.masked_fill(~vis, -math.inf)
        empty = ~vis.any(-1)                                                                        # (Sq)
        lse = torch.logsumexp(S, -1).masked_fill(empty[None], math.inf)                             # the package's marker
        # the forward kernel: exp(S - m) summed in fp32 and rounded to `dtype` for the product with V, the quotient rounded once.  m is the row maximum less
        # 0.17 * variant: an online softmax rounds its probabilities against a running maximum, and another offset is another, nearly independent realisation
        # of that rounding noise -- which is as large in out as out's own rounding (|out| is a random-sign sum of the same terms)
        mx = S.amax(-1, keepdim=True).masked_fill(empty[None, :, None], 0.0) - 0.17 * variant
        Pu = torch.exp(S - mx)
        out = (torch.einsum("hts,shd->thd", Pu.to(dtype).float(), vs) / Pu.sum(-1).masked_fill(empty[None], 1.0).transpose(0, 1)[..., None]).to(dtype)
        sk = s_head[:, None].expand_as(lse)
        off = torch.isneginf(sk)
        f = torch.where(empty[None], torch.zeros_like(lse), torch.where(off, torch.ones_like(lse), torch.sigmoid(lse - sk)))
        lse2 = torch.where(off, lse, torch.where(empty[None], sk, torch.maximum(lse, sk) + torch.log1p(torch.exp(-(lse - sk).abs()))))
        lse_bwd = lse2.masked_fill(empty[None], math.inf)
        if mistake == "lse_without_sink":
            lse2, lse_bwd = lse, lse
        if mistake == "empty_lse_inf":
            lse2 = lse_bwd
        out2 = (out.float() * f.transpose(0, 1)[..., None]).to(dtype)                                # second rounding: the post-pass
        P2 = torch.exp(S - lse_bwd[..., None])
        dV = torch.einsum("hts,thd->shd", P2.to(dtype).float(), dos)
        dP = torch.einsum("thd,shd->hts", dos, vs)
        delta = (dos * out2.float()).sum(-1).transpose(0, 1)                                        # softmax_d (H, Sq)
        dS = P2 * (dP - delta[..., None])
        if m["softcap"] > 0:
            dS = dS * (1 - (S.masked_fill(~vis, 0.0) / m["softcap"]) ** 2)
        dS = dS.to(dtype).float() / math.sqrt(D)
        dq_all[sq_] = torch.einsum("hts,shd->thd", dS, ks)
        dk_all[sk_] = torch.einsum("hts,thd->shd", dS, qs).view(Sk, Hk, g, D).sum(2)
        dv_all[sk_] = dV.view(Sk, Hk, g, D).sum(2)
        delta = delta.masked_fill(empty[None], math.nan)                                            # unwritten on rows without a key
        w = torch.exp(sk - lse_bwd) if mistake != "empty_rows_in_dsink" else torch.exp(sk - lse_bwd.masked_fill(empty[None], 0.0))
        terms = torch.where(w > 0, w * delta, torch.zeros_like(w))
        dsink += (terms if mistake == "dsink_sign" else -terms).double().sum(-1)
        out_all[sq_], lse_all[:, sq_] = out2.float(), lse2
    B = len(m["qlens"])
    lse_out = lse_all if m["packed"] else lse_all.view(H, B, -1).transpose(0, 1)
    return dict(out=out_all.view(shape_q), lse=lse_out.contiguous(), dq=dq_all.to(dtype).float().view(shape_q), dk=dk_all.to(dtype).float().view(shape_k),
                dv=dv_all.to(dtype).float().view(shape_k), dsink=dsink.float())


# ---- the reference's two rules (its tests/cute/test_flash_attn.py: check_tensor_vs_ref, check_dsink_vs_ref), on a fixture that stores max|pt - ref| -----------
def tensor_allowance(ref, err_pt):
    """max|x - ref| <= 2 max|pt - ref| + atol,  atol = 2 max|(ref + 0.3 - 0.3) - ref|."""
    ref = torch.as_tensor(ref, dtype=torch.float32)
    atol = 2 * float((ref + 0.3 - 0.3 - ref).abs().max()) if ref.numel() else 0.0
    return 2 * float(err_pt) + atol


def dsink_allowance(ref, err_pt, softcap, dtype=torch.float32):
    """Per element: |x - ref| <= 2 max|pt - ref| + 2 ulp(ref) (+ 3e-4 under softcap); the ulp is that of ref in the dtype the gradient comes in, as in the
    reference, whose ref has the sink's dtype."""
    r = torch.as_tensor(ref, dtype=torch.float32).to(dtype).abs()
    ulp = (torch.nextafter(r, torch.full_like(r, math.inf)) - r).float()
    return 2 * float(err_pt) + 2 * ulp + (3e-4 if softcap > 0 else 0.0)


def compare(case, got, dtype, sink_dtype=torch.float32):
    """got: {out, dq, dk, dv, dsink[, lse]} tensors in the case's layout.  -> {quantity: worst error / allowance} (in the rule iff <= 1; NaN counts as inf), and
    'lse': the worst |lse - ref| (inf where an infinity or NaN sits in the wrong place)."""
    key = "err_pt_bf16" if dtype == torch.bfloat16 else "err_pt_fp16"
    m = case_meta(case)
    res = {}
    for i, nm in enumerate(QUANTITIES):
        if nm not in got:
            continue
        x, ref = got[nm].detach().float().cpu(), torch.from_numpy(case[nm])
        err = (x - ref).abs()
        allow = dsink_allowance(ref, case[key][i], m["softcap"], sink_dtype) if nm == "dsink" else tensor_allowance(ref, case[key][i])
        ratio = err / allow
        res[nm] = math.inf if not bool(torch.isfinite(x).all()) else float(ratio.max()) if ratio.numel() else 0.0
    if "lse" in got:
        x, ref = got["lse"].detach().float().cpu(), torch.from_numpy(case["lse"])
        same = torch.isfinite(x) == torch.isfinite(ref)
        fin = torch.isfinite(ref)
        bad = not bool(same.all()) or not bool(torch.equal(x[~fin], ref[~fin]))
        res["lse"] = math.inf if bad else float((x[fin] - ref[fin]).abs().max()) if fin.any() else 0.0
    return res
