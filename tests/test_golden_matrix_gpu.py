"""GPU suite on the reference-generated matrix (tests/golden/ref_matrix_*.npz; tests/golden/make_golden.py, tests/test_golden_matrix_cpu.py), with the SHIPPED knobs:
this module is not among the ones tests/conftest.py pins to FA_BWD_GSPLIT=0, so the dK / dV of a split GQA group (fa_api.cpp bwd_gsplit_plan) are what is checked.

Bound = the reference's rule with the reference's recorded baseline (tests/_util.matrix_bound): |out - ref| <= 2 err_pt[out] + 1e-5, gradients <= 3 err_pt[g] + 1e-4
with err_pt = attention_ref in the input dtype on the CPU, stored in the fixture; LSE within 2e-3 (tests/test_fwd_gpu.py); padded rows and keys exactly zero; no
NaN / Inf.  Every case in bf16 and fp16 (the inputs are exact in both), through the binder where the head dim is a multiple of 8 and through the public autograd
API always.  Every fixed-length grouped case runs its backward three times -- default, FA_BWD_GSPLIT=0, forced FA_BWD_GSPLIT=16 -- with the workspace poisoned,
the plan query saying what each run did, and dQ bit for bit the same.

With FA_GOLDEN_MATRIX_RATIOS=<file> the worst err / err_pt ratio per tensor, dtype and knob setting is written there."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests._dropout_model import threshold as dropout_threshold
from tests._util import golden_inputs, load_matrix, matrix_bound, matrix_head_dims, matrix_meta, matrix_names, max_abs

pytestmark = pytest.mark.gpu

FIXED = [("fixed", n) for n in matrix_names("fixed")] + [("long", n) for n in matrix_names("long")]
FIXED_BINDER = [(f, n) for f, n in FIXED if matrix_head_dims(f)[n] % 8 == 0]   # (40 / 160 / 224 included; 59 and 111 reach the kernels through the public API's padding only)
VARLEN = [("varlen", n) for n in matrix_names("varlen")]
DTYPES = [(torch.bfloat16, "bf16"), (torch.float16, "fp16")]
NATIVE_D = (32, 64, 96, 128, 192, 256)   # head dims the dK/dV kernels hold natively (fa_api.cpp head_dim_native): only these split
_WORST = {}                               # (tensor, dtype, knob) -> (err / err_pt, err, err_pt, case)


@pytest.fixture(scope="module")
def be():
    from flash_attn_amd import backend
    return backend


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("FA_GOLDEN_MATRIX_RATIOS")
    if path and _WORST:
        with open(path, "w") as f:
            f.write("# worst err / err_pt per tensor, dtype and knob setting over tests/golden/ref_matrix_*.npz (tests/test_golden_matrix_gpu.py); err = max|kernel - fp32 reference|,\n"
                    "# err_pt = the fixture's max|attention_ref in that dtype on the CPU - fp32 reference|.  Bound: 2 (out) / 3 (gradients), plus a floor of 1e-5 / 1e-4.\n"
                    "# tensor dtype knob                 ratio       err    err_pt  case\n")
            for (t, dn, knob), (r, e, ept, name) in sorted(_WORST.items()):
                f.write("%-4s %-5s %-20s %7.3f %9.3e %9.3e  %s\n" % (t, dn, knob, r, e, ept, name))


def _refs(case):
    return {nm: torch.from_numpy(case[nm]).cuda() for nm in ("out", "dq", "dk", "dv", "lse")}


def _alibi(m):
    return None if m["alibi"] is None else torch.from_numpy(np.asarray(m["alibi"], dtype=np.float32)).cuda()


def _judge(case, name, dn, knob, got, lse=None):
    """got: {tensor: kernel result shaped like the fixture's full tensor}; sampled rows are taken here."""
    m, ref = matrix_meta(case), _refs(case)
    rows = None if m["rows"] is None else torch.from_numpy(m["rows"]).cuda()
    for nm, x in got.items():
        assert torch.isfinite(x.float()).all(), (name, nm, knob)
        x = x.float() if rows is None or nm in ("dk", "dv") else x.float()[:, rows]
        err = max_abs(x, ref[nm])
        bound = matrix_bound(case, nm, dn, float(ref[nm].abs().max()) if ref[nm].numel() else 0.0)
        ept = float(case["err_pt_" + dn][("out", "dq", "dk", "dv").index(nm)])
        print("%s %s %s %s err %.3e err_pt %.3e bound %.3e" % (name, dn, knob, nm, err, ept, bound))
        if ept == ept and ept > 0 and err / ept > _WORST.get((nm, dn, knob), (-1.0,))[0]:
            _WORST[(nm, dn, knob)] = (err / ept, err, ept, name)
        assert err <= bound, (name, nm, dn, knob, err, ept, bound)
    if lse is not None:
        lse = lse if rows is None else lse[:, :, rows]
        fin = torch.isfinite(ref["lse"])
        assert torch.equal(torch.isposinf(lse), ~fin), (name, "lse")
        assert max_abs(lse[fin], ref["lse"][fin]) < 2e-3, (name, "lse", max_abs(lse[fin], ref["lse"][fin]))


def _plan_of(m, dtype, cu_q=None, cu_k=None, total_q=None, total_k=None, D=None):
    """fa_bwd_plan_query for a case's call (tests/test_bwd_schedules_gpu.py _plan_of, with Sq != Sk, windows and packed batches): out[0] = launch kind
    (0 = the dQ + dK/dV pair), out[3] = virtual kv heads a GQA group is split into (0 = unsplit)."""
    from flash_attn_amd import _cabi
    lib = _cabi.load()
    a = _cabi.FaBwdParams()
    a.b, a.h, a.h_k, a.d = m["B"], m["H"], m["Hk"], D or m["D"]
    a.seqlen_q, a.seqlen_k = m["Sq"], m["Sk"]
    a.total_q, a.total_k = (m["B"] * m["Sq"], m["B"] * m["Sk"]) if total_q is None else (total_q, total_k)
    a.dtype = _cabi.FA_DTYPE_BF16 if dtype == torch.bfloat16 else _cabi.FA_DTYPE_FP16
    a.softmax_scale, a.softcap, a.is_causal = m["D"] ** -0.5, m["softcap"], int(m["causal"])
    a.window_left, a.window_right = m["window"]
    if cu_q is not None:
        a.cu_seqlens_q, a.cu_seqlens_k = C.c_void_p(cu_q.data_ptr()), C.c_void_p(cu_k.data_ptr())
    out = (C.c_int32 * 8)()
    assert lib.fa_bwd_plan_query(C.byref(a), out, 8) == 8
    return list(out)


def _forced_split(ratio, cap=16):
    gs = 1
    while gs * 2 <= cap and ratio % (gs * 2) == 0:
        gs *= 2
    return gs if gs > 1 else 0


def _gsplit_settings(knobs, m, dtype, D=None):
    """The knob settings a fixed-length case runs its backward under, as (label, virtual heads the plan reports).  Every grid of the matrix (batch x kv heads x key
    blocks <= 8) stays below the 256 workgroups from which the automatic plan stops splitting even after a split in 8, so by default a group on a native head dim
    is split into the largest power of two (<= 8) that divides it: 4 for ratio 4, 8 for ratio 8, 2 for ratios 2 and 6; ratio 3 and the head dims in between the
    built sizes never are."""
    D = D or m["D"]
    splittable = m["ratio"] % 2 == 0 and D in NATIVE_D
    settings = [("default", None, _forced_split(m["ratio"], 8) if splittable else 0)]
    if m["ratio"] > 1:
        settings += [("FA_BWD_GSPLIT=0", 0, 0), ("FA_BWD_GSPLIT=16", 16, _forced_split(m["ratio"]) if splittable else 0)]
    for label, value, want in settings:
        if value is None:
            knobs.unset("FA_BWD_GSPLIT")
        else:
            knobs.set("FA_BWD_GSPLIT", value)
        plan = _plan_of(m, dtype, D=D)
        assert plan[0] == 0 and plan[3] == want, (label, m["ratio"], D, plan)
        yield label, want


def _split_really_ran(name, m, dkdv):
    """The plan query alone does not show that the split kernels ran: without a workspace the launch falls back to the unsplit ones (fa_api.cpp launch_dkdv_any).
    The partials of a split are rounded to the input dtype before they are summed, so its dK / dV equal the unsplit run's only by accident
    (tests/test_bwd_gsplit_gpu.py asserts the same; a single query row is left out there too)."""
    if m["Sq"] == 1:
        return
    for (label, gs), (dk, dv) in dkdv.items():
        if gs >= 2:
            dk0, dv0 = dkdv["FA_BWD_GSPLIT=0", 0]
            assert not torch.equal(dk, dk0) and not torch.equal(dv, dv0), (name, label, "fell back to the unsplit kernels")


@pytest.mark.parametrize("dtype,dn", DTYPES, ids=[d for _, d in DTYPES])
@pytest.mark.parametrize("family,name", FIXED_BINDER, ids=[n for _, n in FIXED_BINDER])
def test_fixed_length_binder(be, knobs, family, name, dtype, dn):
    """backend.fwd / bwd on every case whose head dim is a multiple of 8."""
    case = load_matrix(family)[name]
    m = matrix_meta(case)
    knobs.set("FA_DEBUG_POISON_WS", 1)
    q, k, v, do = golden_inputs(case, "cuda", dtype)
    alibi, scale = _alibi(m), m["D"] ** -0.5
    out, lse, _, _ = be.fwd(q, k, v, None, alibi, 0.0, scale, m["causal"], m["window"][0], m["window"][1], m["softcap"], False, None)
    _judge(case, name, dn, "forward", {"out": out}, lse)
    dq0, dkdv = None, {}
    for label, gs in _gsplit_settings(knobs, m, dtype):
        dq, dk, dv, _ = be.bwd(do, q, k, v, out, lse, None, None, None, alibi, 0.0, scale, m["causal"], m["window"][0], m["window"][1], m["softcap"], False, None, None)
        _judge(case, name, dn, label, {"dq": dq, "dk": dk, "dv": dv})
        dq0, dkdv[label, gs] = dq if dq0 is None else dq0, (dk, dv)
        assert torch.equal(dq, dq0), (name, label, "dq is not the split's")
    _split_really_ran(name, m, dkdv)


@pytest.mark.parametrize("dtype,dn", DTYPES, ids=[d for _, d in DTYPES])
@pytest.mark.parametrize("family,name", FIXED, ids=[n for _, n in FIXED])
def test_fixed_length_public_api(knobs, family, name, dtype, dn):
    """flash_attn_func (+ the kv-packed / qkv-packed forms where the shapes allow) with autograd: every case, head dims 40 / 59 / 111 included (59 and 111 are padded
    to 64 and 112 by the interface: 64 is a native head dim, so the grouped D = 59 case runs a split backward by default)."""
    from flash_attn_amd import flash_attn_interface as fi
    case = load_matrix(family)[name]
    m = matrix_meta(case)
    knobs.set("FA_DEBUG_POISON_WS", 1)
    kw = dict(causal=m["causal"], window_size=m["window"], softcap=m["softcap"], alibi_slopes=_alibi(m))
    Dk = -(-m["D"] // 8) * 8
    dq0, dkdv = None, {}
    for label, gs in _gsplit_settings(knobs, m, dtype, D=Dk):
        q, k, v, do = golden_inputs(case, "cuda", dtype)
        q, k, v = (t.requires_grad_() for t in (q, k, v))
        out, lse, _ = fi.flash_attn_func(q, k, v, return_attn_probs=True, **kw)
        dq, dk, dv = torch.autograd.grad(out, (q, k, v), do)
        _judge(case, name, dn, "api " + label, {"out": out.detach(), "dq": dq, "dk": dk, "dv": dv}, lse.detach())
        dq0, dkdv[label, gs] = dq if dq0 is None else dq0, (dk, dv)
        assert torch.equal(dq, dq0), (name, label, "dq is not the split's")
    _split_really_ran(name, m, dkdv)
    knobs.unset("FA_BWD_GSPLIT")
    if m["Sq"] == m["Sk"]:
        q, k, v, do = golden_inputs(case, "cuda", dtype)
        q.requires_grad_()
        kv = torch.stack([k, v], dim=2).requires_grad_()
        out = fi.flash_attn_kvpacked_func(q, kv, **kw)
        dq, dkv = torch.autograd.grad(out, (q, kv), do)
        _judge(case, name, dn, "api kvpacked", {"out": out.detach(), "dq": dq, "dk": dkv[:, :, 0], "dv": dkv[:, :, 1]})
        if m["H"] == m["Hk"]:
            qkv = torch.stack([q.detach(), k, v], dim=2).requires_grad_()
            out = fi.flash_attn_qkvpacked_func(qkv, **kw)
            (dqkv,) = torch.autograd.grad(out, (qkv,), do)
            _judge(case, name, dn, "api qkvpacked", {"out": out.detach(), "dq": dqkv[:, :, 0], "dk": dqkv[:, :, 1], "dv": dqkv[:, :, 2]})


def _unpad(case, dtype):
    from flash_attn_amd.bert_padding import unpad_input
    q, k, v, do = golden_inputs(case, "cuda", dtype)
    qmask, kmask = torch.from_numpy(case["qmask"]).cuda(), torch.from_numpy(case["kmask"]).cuda()
    qu, iq, cu_q, mq, _ = unpad_input(q, qmask)
    ku, ik, cu_k, mk, _ = unpad_input(k, kmask)
    vu, dou = unpad_input(v, kmask)[0], unpad_input(do, qmask)[0]
    return qu, ku, vu, dou, iq, ik, cu_q.int().contiguous(), cu_k.int().contiguous(), int(mq), int(mk)


def _judge_packed(case, name, dn, knob, out_u, dq_u, dk_u, dv_u, lse_u, iq, ik):
    """Pads the packed results back with the project's pad_input and compares them with the padded fixture: the padded rows and keys are zero on both sides."""
    from flash_attn_amd.bert_padding import pad_input
    m = matrix_meta(case)
    got = {"out": pad_input(out_u, iq, m["B"], m["Sq"]), "dq": pad_input(dq_u, iq, m["B"], m["Sq"]), "dk": pad_input(dk_u, ik, m["B"], m["Sk"]),
           "dv": pad_input(dv_u, ik, m["B"], m["Sk"])}
    qmask, kmask = torch.from_numpy(case["qmask"]).cuda(), torch.from_numpy(case["kmask"]).cuda()
    for nm, mask in (("out", qmask), ("dq", qmask), ("dk", kmask), ("dv", kmask)):
        assert torch.all(got[nm][~mask] == 0), (name, nm, "padded positions")
    _judge(case, name, dn, knob, got)
    ref_l, start = torch.from_numpy(case["lse"]).cuda(), 0
    for b in range(m["B"]):   # lse_u: (H, total_q)
        n = int(qmask[b].sum())
        a, r = lse_u[:, start:start + n], ref_l[b, :, :n]
        fin = torch.isfinite(r)
        assert torch.equal(torch.isposinf(a), ~fin) and max_abs(a[fin], r[fin]) < 2e-3, (name, "lse", b)
        start += n


@pytest.mark.parametrize("dtype,dn", DTYPES, ids=[d for _, d in DTYPES])
@pytest.mark.parametrize("family,name", VARLEN, ids=[n for _, n in VARLEN])
def test_packed_batches(be, knobs, family, name, dtype, dn):
    """Padded batches of the reference's generate_random_padding_mask, unpadded with the project's bert_padding: varlen_fwd / varlen_bwd (head dim a multiple of 8)
    and flash_attn_varlen_func (all).  A packed batch is never split."""
    from flash_attn_amd import flash_attn_interface as fi
    case = load_matrix(family)[name]
    m = matrix_meta(case)
    knobs.set("FA_DEBUG_POISON_WS", 1)
    qu, ku, vu, dou, iq, ik, cu_q, cu_k, mq, mk = _unpad(case, dtype)
    scale, (wl, wr) = m["D"] ** -0.5, m["window"]
    assert _plan_of(m, dtype, cu_q, cu_k, qu.shape[0], ku.shape[0], D=-(-m["D"] // 8) * 8)[3] == 0
    if m["D"] % 8 == 0:
        out, lse, _, _ = be.varlen_fwd(qu, ku, vu, None, cu_q, cu_k, None, None, None, None, mq, mk, 0.0, scale, False, m["causal"], wl, wr, 0.0, False, None)
        dq, dk, dv, _ = be.varlen_bwd(dou, qu, ku, vu, out, lse, None, None, None, cu_q, cu_k, None, mq, mk, 0.0, scale, False, m["causal"], wl, wr, 0.0, False, None, None)
        _judge_packed(case, name, dn, "varlen", out, dq, dk, dv, lse, iq, ik)
    qu, ku, vu = (t.requires_grad_() for t in (qu, ku, vu))
    out, lse, _ = fi.flash_attn_varlen_func(qu, ku, vu, cu_q, cu_k, mq, mk, causal=m["causal"], window_size=m["window"], return_attn_probs=True)
    dq, dk, dv = torch.autograd.grad(out, (qu, ku, vu), dou)
    _judge_packed(case, name, dn, "api varlen", out.detach(), dq, dk, dv, lse.detach(), iq, ik)


FEATURE_CASES = [n for n in matrix_names("fixed") if n.startswith(("softcap_", "alibi_"))]


def _oracle_check(got, ref, what):
    """The bound of tests/test_bwd_gpu.py test_softcap_backward_vs_oracle: out within 2e-2, gradients within 3e-2 * max(1, max|ref|) of the fp64 oracle."""
    for nm, x in got.items():
        r = torch.from_numpy(ref[nm])
        assert torch.isfinite(x.float()).all(), (what, nm)
        err = max_abs(x.float().cpu(), r)
        print(what, nm, "err %.3e max|ref| %.3e" % (err, float(r.abs().max())))
        assert err < (2e-2 if nm == "out" else 3e-2 * max(1.0, float(r.abs().max()))), (what, nm, err)


@pytest.mark.parametrize("dtype,dn", DTYPES, ids=[d for _, d in DTYPES])
@pytest.mark.parametrize("name", FEATURE_CASES)
def test_softcap_and_alibi_under_the_split_vs_oracle(be, knobs, name, dtype, dn):
    """tests/test_bwd_gsplit_gpu.py compares its softcap / ALiBi shapes with the unsplit kernels only: here the automatic and the forced split of the ratio-4 cases
    against the fp64 oracle itself."""
    from oracle import attention_oracle as orc
    case = load_matrix("fixed")[name]
    m = matrix_meta(case)
    assert m["ratio"] == 4
    knobs.set("FA_DEBUG_POISON_WS", 1)
    q, k, v, do = golden_inputs(case, "cuda", dtype)
    alibi, scale, (wl, wr) = _alibi(m), m["D"] ** -0.5, m["window"]
    o_ref, _ = orc.attention_fwd(q, k, v, scale, m["causal"], m["window"], m["softcap"], m["alibi"])
    g_ref = orc.attention_bwd(do, q, k, v, None, None, scale, m["causal"], m["window"], m["softcap"], m["alibi"])
    ref = dict(out=o_ref, dq=g_ref[0], dk=g_ref[1], dv=g_ref[2])
    out, lse, _, _ = be.fwd(q, k, v, None, alibi, 0.0, scale, m["causal"], wl, wr, m["softcap"], False, None)
    for label, value, want in (("default", None, None), ("FA_BWD_GSPLIT=16", 16, 4)):
        knobs.unset("FA_BWD_GSPLIT") if value is None else knobs.set("FA_BWD_GSPLIT", value)
        plan = _plan_of(m, dtype)
        assert plan[0] == 0 and (plan[3] >= 2 if want is None else plan[3] == want), (label, plan)
        dq, dk, dv, _ = be.bwd(do, q, k, v, out, lse, None, None, None, alibi, 0.0, scale, m["causal"], wl, wr, m["softcap"], False, None, None)
        _oracle_check(dict(out=out, dq=dq, dk=dk, dv=dv), ref, (name, dn, label))


@pytest.mark.parametrize("dtype,dn", DTYPES, ids=[d for _, d in DTYPES])
@pytest.mark.parametrize("shape", [(2, 113, 203, 8, 2, 64, True, 0.17), (1, 256, 512, 8, 1, 128, False, 0.3)], ids=["ratio4_causal_113x203_d64", "ratio8_full_256x512_d128"])
def test_dropout_under_the_split_vs_oracle(be, knobs, shape, dtype, dn):
    """Dropout on a split group against the fp64 oracle, the keep-mask taken from the forward's return_softmax payload as in tests/test_dropout_gpu.py (the oracle's
    dropout branch is pinned to the reference by tests/golden/dropout_ref_cases.npz, tests/test_oracle_cpu.py): the virtual heads of a split group must regenerate
    the mask of their REAL query heads."""
    from oracle import attention_oracle as orc
    B, Sq, Sk, H, Hk, D, causal, p = shape
    knobs.set("FA_DEBUG_POISON_WS", 1)
    g = torch.Generator().manual_seed(Sq * 3 + Sk)
    q, k, v, do = (torch.randn(*s, generator=g).to("cuda", dtype) for s in ((B, Sq, H, D), (B, Sk, Hk, D), (B, Sk, Hk, D), (B, Sq, H, D)))
    scale = D ** -0.5
    torch.manual_seed(3)
    out, lse, rv, rng = be.fwd(q, k, v, None, None, p, scale, causal, -1, -1, 0.0, True, None)
    keep = (rv.to(torch.int32) <= dropout_threshold(p)).cpu().numpy()
    o_ref, _ = orc.attention_fwd(q, k, v, scale, causal, (-1, -1), 0.0, None, p, keep)
    g_ref = orc.attention_bwd(do, q, k, v, None, None, scale, causal, (-1, -1), 0.0, None, p, keep)
    ref = dict(out=o_ref, dq=g_ref[0], dk=g_ref[1], dv=g_ref[2])
    m = dict(B=B, Sq=Sq, Sk=Sk, H=H, Hk=Hk, D=D, causal=causal, window=(-1, -1), softcap=0.0)
    for label, value, want in (("default", None, None), ("FA_BWD_GSPLIT=16", 16, H // Hk)):
        knobs.unset("FA_BWD_GSPLIT") if value is None else knobs.set("FA_BWD_GSPLIT", value)
        plan = _plan_of(m, dtype)
        assert plan[0] == 0 and (plan[3] >= 2 if want is None else plan[3] == want), (label, plan)
        dq, dk, dv, _ = be.bwd(do, q, k, v, out, lse, None, None, None, None, p, scale, causal, -1, -1, 0.0, False, None, rng)
        _oracle_check(dict(out=out, dq=dq, dk=dk, dv=dv), ref, ("dropout", shape, dn, label))
