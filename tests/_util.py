"""Shared helpers for the parity tests (test infrastructure only)."""
from __future__ import annotations

import math

import numpy as np
import torch


def bf16_bits_to_f32(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def golden_inputs(case, device=None, dtype=torch.bfloat16):
    """q, k, v, do tensors of a golden case (exactly bf16-representable values)."""
    out = []
    for nm in ("q", "k", "v", "do"):
        t = torch.from_numpy(bf16_bits_to_f32(case[nm + "_bf16bits"]).copy())
        out.append(t.to(device=device, dtype=dtype) if device is not None else t)
    return out


def case_meta(case):
    B, Sq, Sk, H, Hk, D, causal, wl, wr = [int(x) for x in case["meta"]]
    return dict(B=B, Sq=Sq, Sk=Sk, H=H, Hk=Hk, D=D, causal=bool(causal), window=(wl, wr),
                softcap=float(case["softcap"][0]),
                alibi=case.get("alibi_slopes"))


def local_mask_torch(sq, sk, window, device):
    """True = masked; same predicate as the oracle's visible_mask (bottom-right aligned)."""
    i = torch.arange(sq, device=device)[:, None]
    j = torch.arange(sk, device=device)[None, :]
    wl, wr = window
    masked = torch.zeros(sq, sk, dtype=torch.bool, device=device)
    if wr >= 0:
        masked |= j > i + (sk - sq) + wr
    if wl >= 0:
        masked |= j < i + (sk - sq) - wl
    return masked


def attention_torch(q, k, v, causal=False, window=(-1, -1), softmax_scale=None, upcast=True, reorder=False):
    """Plain PyTorch attention on the tensors' device (large-size reference / low-precision baseline).

    upcast=True: fp32 math (the reference point); upcast=False: math in the input dtype (the
    'PyTorch baseline' whose error calibrates the tolerance, as in the reference's tests).
    Returns out (B,Sq,H,D) in the input dtype and lse (B,H,Sq) fp32.
    """
    dt = q.dtype
    if causal:
        window = (window[0], 0)
    if upcast:
        q, k, v = q.float(), k.float(), v.float()
    B, Sq, H, D = q.shape
    Sk, Hk = k.shape[1], k.shape[2]
    g = H // Hk
    k = k.repeat_interleave(g, dim=2)
    v = v.repeat_interleave(g, dim=2)
    scale = D ** -0.5 if softmax_scale is None else softmax_scale
    if reorder:
        s = torch.einsum("bthd,bshd->bhts", q, k * scale)
    else:
        s = torch.einsum("bthd,bshd->bhts", q * scale, k)
    if window[0] >= 0 or window[1] >= 0:
        wl = -1 if window[0] >= Sk else window[0]
        wr = -1 if window[1] >= Sk else window[1]
        m = local_mask_torch(Sq, Sk, (wl, wr), q.device)
        s = s.masked_fill(m, float("-inf"))
        dead = m.all(dim=-1)
    else:
        dead = None
    lse = torch.logsumexp(s.float(), dim=-1)
    p = torch.softmax(s, dim=-1)
    if dead is not None:
        p = p.masked_fill(dead[None, None, :, None], 0.0)
        lse = lse.masked_fill(dead[None, None, :], float("inf"))
    o = torch.einsum("bhts,bshd->bthd", p.to(v.dtype), v)
    return o.to(dt), lse


def max_abs(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


MATRIX_FAMILIES = ("fixed", "varlen", "long")


def matrix_files(family):
    import glob
    import os
    return sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_matrix_%s_*.npz" % family)))


def matrix_names(family):
    """Case names of one family of tests/golden/ref_matrix_<family>_NN.npz (tests/golden/make_golden.py MATRIX), without reading the arrays."""
    names = []
    for path in matrix_files(family):
        with np.load(path) as z:
            for k in z.files:
                if "/" in k and k.split("/")[0] not in names:
                    names.append(k.split("/")[0])
    return names


def matrix_head_dims(family):
    """{case name: head dim}, from the meta arrays alone."""
    dims = {}
    for path in matrix_files(family):
        with np.load(path) as z:
            dims.update({k.split("/")[0]: int(z[k][5]) for k in z.files if k.endswith("/meta")})
    return dims


_MATRIX_CACHE = {}


def load_matrix(family):
    """{case name: {key: array}} of one family; arrays the generator cut into <key>__partN pieces are joined again."""
    if family in _MATRIX_CACHE:
        return _MATRIX_CACHE[family]
    flat = {}
    for path in matrix_files(family):
        with np.load(path) as z:
            flat.update({k: z[k] for k in z.files})
    for k in [k for k in flat if k.endswith("__shape")]:
        base = k[: -len("__shape")]
        n = sum(1 for x in flat if x.startswith(base + "__part"))
        flat[base] = np.concatenate([flat.pop("%s__part%d" % (base, i)) for i in range(n)]).reshape(tuple(flat.pop(k)))
    cases = {}
    for k, a in flat.items():
        if "/" in k:
            cases.setdefault(k.split("/")[0], {})[k.split("/", 1)[1]] = a
    cases["README"] = str(flat["README"])
    _MATRIX_CACHE[family] = cases
    return cases


def matrix_meta(case):
    m = case_meta(case)
    m["ratio"] = m["H"] // m["Hk"]
    m["rows"] = case.get("rows")
    m["bwd_from_oracle"] = "bwd_from_oracle" in case
    m["packed"] = "qmask" in case
    return m


def matrix_bound(case, tensor, dtype_name, ref_absmax=None, err_pt=None):
    """The reference's rule with the reference's recorded baseline (tests/test_flash_attn.py:1130-1132): |out - ref| <= 2 err_pt[out] + 1e-5, gradients
    <= 3 err_pt[g] + 1e-4, err_pt = the fixture's err_pt_<dtype> (attention_ref in that dtype on the CPU) unless the caller brings its own.  Softcap cases have no
    differentiable reference in the input dtype (in-place tanh): their gradients take the bound of test_bwd_gpu.py test_softcap_backward_vs_oracle."""
    i = ("out", "dq", "dk", "dv").index(tensor)
    e = float(case["err_pt_" + dtype_name][i]) if err_pt is None else err_pt
    if i == 0:
        return 2 * e + 1e-5
    if "bwd_from_oracle" in case:
        return 3e-2 * max(1.0, ref_absmax)
    return 3 * e + 1e-4
