"""The merge of partial attention results in float64 numpy, and the acceptance rule of the reference's test_flash_attn_combine (test infrastructure only).

    lse = m + log(sum_live exp(lse_i - m)),  out = sum_live exp(lse_i - lse) * o_i,   live = lse_i finite,  m = max of the live lse_i

A row with no live partial has out = 0 and lse = `empty` (-inf: FA3's flash_attn_combine, +inf: this package's merge_attn_states).  The o rows of empty partials
are never multiplied: NaN there does not reach the reference either."""
import numpy as np
import torch


def combine_ref64(o, lse, empty=-np.inf):
    """o (S, ..., D), lse (S, ...): numpy arrays or CPU tensors of any float dtype -> (out, lse) float64."""
    o = o.double().numpy() if isinstance(o, torch.Tensor) else np.asarray(o, dtype=np.float64)
    lse = lse.double().numpy() if isinstance(lse, torch.Tensor) else np.asarray(lse, dtype=np.float64)
    live = np.isfinite(lse)
    dead = ~live.any(0)
    m = np.where(dead, 0.0, np.where(live, lse, -np.inf).max(0))
    e = np.where(live, np.exp(np.where(live, lse, 0.0) - m), 0.0)
    s = np.where(dead, 1.0, e.sum(0))
    out = (np.where(live[..., None], o, 0.0) * (e / s)[..., None]).sum(0)
    return out, np.where(dead, empty, m + np.log(s))


def within_reference_rule(out, lse, out_ref, lse_ref, dtype):
    """(ok, figures): lse allclose(atol = rtol = 1e-5) with equal infinities equal; max|out - ref| <= 2 max|ref.to(dtype) - ref|, or allclose(1e-5) to ref.to(dtype).
    out / lse: tensors (any device); out_ref / lse_ref: float64 (or fp32) numpy arrays."""
    out = out.detach().double().cpu().numpy()
    out_ref = np.asarray(out_ref, dtype=np.float64)
    rounded = torch.from_numpy(out_ref).to(dtype).double().numpy()
    err, base = float(np.abs(out - out_ref).max(initial=0.0)), float(np.abs(rounded - out_ref).max(initial=0.0))
    ok_out = bool(np.isfinite(out).all()) and (err <= 2 * base or bool(np.allclose(out, rounded, atol=1e-5, rtol=1e-5)))
    ok_lse = True
    lse_err = 0.0
    if lse is not None:
        lse = lse.detach().double().cpu().numpy()
        lse_ref = np.asarray(lse_ref, dtype=np.float64)
        ok_lse = bool(np.allclose(lse, lse_ref, atol=1e-5, rtol=1e-5))
        fin = np.isfinite(lse_ref)
        lse_err = float(np.abs(lse[fin] - lse_ref[fin]).max(initial=0.0)) if ok_lse else float("nan")
    return ok_out and ok_lse, dict(out_err=err, rounding=base, lse_err=lse_err, ok_out=ok_out, ok_lse=ok_lse)


def load_cases(path):
    z = np.load(path)
    names = sorted({k.split("/")[0] for k in z.files})
    return {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in names}
