"""The layout helper (tests/_layouts.py) can fail, and its case table is complete.  No GPU.

  * every layout's view holds the data, everything else in the arena is poison, strides are multiples of 16 bytes, bases 16-byte aligned;
  * the conditions of the "all different" assignments A2 / A3 hold on the strides the census shapes produce;
  * mutants: a plain torch attention that addresses its tensors through as_strided, once correctly and once with a deliberately wrong (batch, row, head)
    triple, is reported -- by a NaN or by a bitwise difference -- under A2 or A3.  What A1 ("as callers do") cannot see is stated in A1_BLIND, with the reason;
  * coverage: every kernel family of the census that takes a tensor stride is in the layout case list at every head-dim pitch the library builds for it.
"""
import itertools

import pytest
import torch

from tests import _kernel_census as kc
from tests import _layouts as L

B, H, HK = 2, 4, 2


# ---- the layouts ---------------------------------------------------------------------------------------------------------------------------------
_PLACED = [(l, s, d) for l in L.LAYOUTS if l != "fused_proj" for s in ((2, 5, 3, 16), (7, 3, 16)) for d in (torch.bfloat16, torch.float16, torch.float8_e4m3fn)
           if not (len(s) == 3 and l == "bcast_b")]   # (a packed tensor has no batch dimension to expand)


@pytest.mark.parametrize("layout,shape,dtype", _PLACED, ids=[f"{l}-{len(s)}d-{str(d).split('.')[-1]}" for l, s, d in _PLACED])
def test_layout_places_the_data_and_poisons_the_rest(layout, shape, dtype):
    g = torch.Generator().manual_seed(1)
    data = torch.randn(shape, generator=g).to(dtype)
    for kind in ("input", "output"):
        if kind == "output" and (layout == "bcast_b" or data.element_size() != 2):   # outputs are bf16 / fp16 and never expanded
            continue
        a, v = L.place(layout, data=data) if kind == "input" else L.place(layout, shape=shape, dtype=dtype, kind="output")
        if kind == "output":
            assert bool((a.bits() == L.SENTINEL).all())
            v.copy_(data)
        want = data[:1].expand(shape) if layout == "bcast_b" else data
        assert torch.equal(v.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8))
        at = a.view_mask().nonzero()
        assert at.numel() == (data[:1].numel() if layout == "bcast_b" else data.numel())
        assert a.outside_intact()
        chunk = 16 // data.element_size()
        assert all(s % chunk == 0 for s in v.stride()[:-1]) and v.stride(-1) == 1
        assert v.data_ptr() % 16 == 0
        if layout == "bshd":
            assert v.data_ptr() % 32 == 16, "the contiguous arena is deliberately not 32-byte aligned"
        rows = L.PAD_ROWS * v.stride(-3)
        assert int(at.min()) >= rows and a.flat.numel() - 1 - int(at.max()) >= rows, "128 rows' worth of poison on both sides"
        if kind == "input":
            assert a.unchanged()
            a.bits()[3] = 0
            assert not a.unchanged() and not a.outside_intact()


def test_fused_projection_shares_one_arena():
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(2, s, h, 16, generator=g).to(torch.bfloat16) for s, h in ((5, 4), (7, 2), (7, 2)))
    a, (qv, kv, vv) = L.place_fused(datas=[q, k, v])
    assert torch.equal(qv, q) and torch.equal(kv, k) and torch.equal(vv, v) and a.outside_intact() and a.unchanged()
    assert L.triple(qv) == L.triple(kv) == L.triple(vv) == (7 * 8 * 16, 8 * 16, 16)
    assert kv.data_ptr() - qv.data_ptr() == 4 * 16 * 2 and vv.data_ptr() - qv.data_ptr() == 6 * 16 * 2
    assert torch.isnan(a.buf[:, 5:, :4 * 16].float()).all(), "the rows q does not use are poison"


# ---- A2 / A3 on the census shapes ------------------------------------------------------------------------------------------------------------------
def _census_shapes():
    """(Sq, Sk, D, Dv) of the attention rows of the census (tests/_kernel_census.py: B = 2, heads 4 / 2)."""
    shapes = set()
    for r in kc.RECIPES:
        if r["kind"] == "attn":
            shapes.add((r["sq"], r["sk"], r["d"], r["d"]))
        elif r["kind"] == "dv":
            shapes.add((r["sq"], r["sk"], 192, 128))
        elif r["kind"] in ("fp8",):
            shapes.add((r["sq"], r["sk"], r["d"], r["d"]))
    return sorted(shapes)


def _meta_call(assignment, sq, sk, d, dv):
    q, k, v, o = (B, sq, H, d), (B, sk, HK, d), (B, sk, HK, dv), (B, sq, H, dv)
    M = lambda s: torch.empty(s, dtype=torch.bfloat16, device="meta")
    views, _ = L.place_call(assignment, dict(q=M(q), k=M(k), v=M(v), dout=M(o)), dict(out=o, dq=q, dk=k, dv=v), dtype=torch.bfloat16, device="meta")
    return views


@pytest.mark.parametrize("assignment", ["A2", "A3"])
def test_all_different_assignments_are_all_different(assignment):
    shapes = _census_shapes()
    assert len(shapes) >= 10
    for sq, sk, d, dv in shapes:
        t = {r: L.triple(x) for r, x in _meta_call(assignment, sq, sk, d, dv).items()}
        for a, b in (("k", "v"), ("dout", "out"), ("dq", "q"), ("dk", "k"), ("dv", "v")):
            assert t[a] != t[b], (assignment, (sq, sk, d, dv), a, b, t[a])
        fwd, bwd = ("q", "k", "v", "out"), ("dout", "q", "k", "v", "out", "dq", "dk", "dv")   # the tensors of the forward call, of the backward call
        for call in (fwd, bwd):
            for a, b in itertools.combinations(call, 2):
                assert t[a] != t[b], (assignment, (sq, sk, d, dv), a, b, t[a])
        assert all(s % 8 == 0 for tr in t.values() for s in tr)


def test_every_role_meets_three_noncontiguous_layouts():
    for role in L.ATTN_ROLES + ("kcache", "vcache", "knew", "vnew"):
        seen = {L.ASSIGNMENTS[a][role] for a in ("A1", "A2", "A3")}
        assert len(seen) == 3 and "bshd" not in seen, (role, seen)
    for role in ("kcache", "vcache"):
        seen = {L.PAGED[a][role] for a in ("A1", "A2", "A3")}
        assert len(seen) == 3 and "bshd" not in seen, (role, seen)
    assert L.ASSIGNMENTS["A4"]["k"] == L.ASSIGNMENTS["A4"]["v"] == "bcast_b" and L.ASSIGNMENTS["A4"]["q"] == "sbhd"
    assert L.ASSIGNMENTS["A1"]["out"] == "bhsd" and L.ASSIGNMENTS["A1"]["dout"] == "sbhd"
    assert all(L.ASSIGNMENTS["A1"][r] == "fused_proj" for r in ("q", "k", "v", "dq", "dk", "dv"))


# ---- mutants -------------------------------------------------------------------------------------------------------------------------------------
SQ, SK, D = 5, 7, 16


def _mutant_v_rs_from_k(s):
    s["v"][1][1] = s["k"][1][1]


def _mutant_dout_strides_from_out(s):
    s["dout"][1][:3] = s["out"][1][:3]


def _mutant_dk_strides_from_k(s):
    s["dk"][1][:3] = s["k"][1][:3]


def _mutant_head_stride_is_d(s):
    for role in s:
        s[role][1][2] = s[role][0][3]


def _mutant_batch_stride_is_s_rs(s):
    for role in s:
        s[role][1][0] = s[role][0][1] * s[role][1][1]


def _mutant_store_past_d(s):
    s["out"][0][3] += 8


def _mutant_read_past_s(s):
    s["k"][0][1] += 1
    s["v"][0][1] += 1


MUTANTS = {"v_rs_from_k": _mutant_v_rs_from_k, "dout_strides_from_out": _mutant_dout_strides_from_out, "dk_strides_from_k": _mutant_dk_strides_from_k,
           "head_stride_is_d": _mutant_head_stride_is_d, "batch_stride_is_s_rs": _mutant_batch_stride_is_s_rs, "store_past_d": _mutant_store_past_d,
           "read_past_s": _mutant_read_past_s}
# What A1 cannot see: there q, k and v are column slices of ONE arena and dq, dk and dv of another of the same shape, so k and v share their row stride (V read with K's
# row stride reads V) and dk has k's whole triple (dK written with K's strides lands in dk).  That is the layout callers send most, and the reason A2 / A3 exist.
A1_BLIND = {"v_rs_from_k", "dk_strides_from_k"}


def _strided_attention(views, mutate):
    """Forward and backward of plain attention in fp32, every tensor addressed as base + strides through as_strided -- the strides the mutant left."""
    spec = {r: [list(v.shape), list(v.stride()), v.storage_offset()] for r, v in views.items()}
    mutate(spec)
    t = {r: views[r].as_strided(*spec[r]) for r in views}
    q, k, v = (t[r].float().requires_grad_() for r in ("q", "k", "v"))
    g = H // HK
    s = torch.einsum("bqhd,bkhd->bhqk", q, k.repeat_interleave(g, 2)) * D ** -0.5
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v.repeat_interleave(g, 2))
    t["out"][..., :D] = o.detach().to(torch.bfloat16)
    t["out"][..., D:] = 0
    o.backward(t["dout"].float())
    for role, x in (("dq", q), ("dk", k), ("dv", v)):
        rows = t[role].shape[1]
        t[role].copy_(x.grad[:, :rows].to(torch.bfloat16))


def _run(assignment, mutate, data):
    q, k, v, do = data
    views, arenas = L.place_call(assignment, dict(q=q, k=k, v=v, dout=do), dict(out=do.shape, dq=q.shape, dk=k.shape, dv=v.shape), dtype=torch.bfloat16)
    _strided_attention(views, mutate)
    return views, arenas


def _reported(assignment, mutate, data, want):
    views, arenas = _run(assignment, mutate, data)
    for role in L.OUTPUT_ROLES:
        if torch.isnan(views[role].float()).any() or not torch.equal(views[role].view(torch.int16), want[role].view(torch.int16)):
            return True
    return not all(a.outside_intact() and (a.kind == "output" or a.unchanged()) for a in arenas)


@pytest.fixture(scope="module")
def problem():
    g = torch.Generator().manual_seed(3)
    data = tuple(torch.randn(B, s, h, D, generator=g).to(torch.bfloat16) for s, h in ((SQ, H), (SK, HK), (SK, HK), (SQ, H)))
    q, k, v, do = data
    views = dict(q=q, k=k, v=v, dout=do, out=torch.empty_like(do), dq=torch.empty_like(q), dk=torch.empty_like(k), dv=torch.empty_like(v))
    _strided_attention(views, lambda s: None)
    return data, views


@pytest.mark.parametrize("assignment", ["A1", "A2", "A3"])
def test_the_unmutated_attention_is_not_reported(problem, assignment):
    data, want = problem
    assert not _reported(assignment, lambda s: None, data, want)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_mutant_is_reported(problem, name):
    data, want = problem
    seen = {a for a in ("A1", "A2", "A3") if _reported(a, MUTANTS[name], data, want)}
    assert seen & {"A2", "A3"}, (name, seen)
    assert ("A1" not in seen) == (name in A1_BLIND), (name, seen)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------------------
def test_every_strided_kernel_family_is_in_the_case_list_at_every_pitch():
    rows = L.select_cases(kc.RECIPES)
    assert len({r["id"] for r in rows}) == len(rows)
    need = {L.pitch(k) for r in kc.RECIPES for k in r["keys"] if k[0] not in L.STRIDELESS}
    have = {L.pitch(k) for r in rows for k in r["keys"]}
    assert not need - have, sorted(need - have)
    families = {k[0] for r in kc.RECIPES for k in r["keys"]}
    assert set(L.STRIDELESS) <= families and len(families - {k[0] for r in rows for k in r["keys"]}) == len(L.STRIDELESS)
    for r in rows:
        a = L.assignments_of(r)
        assert a[:3] == ("A1", "A2", "A3")
        if r["kind"] in ("kvcache", "mla", "fp8", "fp8kv") or (r["kind"] == "attn" and not r["varlen"] and not any(k[0].startswith("fa_bwd") for k in r["keys"])):
            assert "A4" in a, r["id"]
