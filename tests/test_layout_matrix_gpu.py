"""Every kernel on strided tensor layouts (tests/_layouts.py; the CPU half, tests/test_layouts_cpu.py, proves that the helper reports a wrong stride and that the
case list holds every kernel family with a tensor stride at every head-dim pitch).

Cases are census recipes by id (tests/_kernel_census.py: their shapes, knobs and launch-log keys) plus a few derived rows (_layouts.DERIVED).  Each case runs
under the assignments A1 - A3, forward and cache rows also under A4 (k / v expanded over the batch), through the ctypes binder:

  1. the call on .contiguous() copies with library-allocated outputs;
  2. the same call on the arena views, outputs into arena views (the generator re-seeded before each call: dropout draws the same mask);
  3. the launch logs of both hold the recipe's keys and are EQUAL: a layout does not change the dispatch at these sizes;
  4. every output view -- and LSE, softmax_d, the dropout payload -- equals the contiguous call's bit for bit: a layout changes addresses, not arithmetic;
  5. every output arena still holds its sentinel outside the view; 6. every input arena is unchanged and no output holds a NaN; 7. the contiguous output is
  finite and not constant.

Then a handful of autograd cases on the default dispatch, and the alignment contract of the 16-bit C ABI through the binder (nothing is enqueued)."""
import math
import zlib

import pytest
import torch

from tests import _kernel_census as kc
from tests import _layouts as L

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
B, H, HK = 2, 4, 2
DEV = "cuda"
ROWS = L.select_cases(kc.RECIPES)
CASES = [(r, a) for r in ROWS for a in L.assignments_of(r)]


class _Log:
    """The launch log of everything a call runs (the ctypes binder checks every launching C call's return code with _cabi.check, which here reads the log first)."""

    def __init__(self, knobs, monkeypatch, row_knobs):
        from flash_attn_amd import _cabi, backend
        self.names, self.be, self.cabi = [], backend, _cabi
        for name, value in dict(row_knobs, FA_DEBUG_LAUNCH_LOG=1, FA_DEBUG_POISON_WS=1).items():
            knobs.set(name, value)
        check = _cabi.check

        def logged_check(rc):
            self.names.extend(backend.launch_log())
            return check(rc)
        monkeypatch.setattr(_cabi, "check", logged_check)

    def take(self):
        names, self.names = self.names, []
        return names


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _execute(log, row, assignment, inputs, outputs, call, dtype, paged=False, inout=()):
    """inputs {role: tensor}, outputs {role: shape}; call(tensors by role, outputs None = library-allocated) -> {name: result}.  Steps 1 - 7 of the module text."""
    views, arenas = L.place_call(assignment, inputs, outputs, dtype=dtype, device=DEV, paged=paged)
    contig = {r: None if v is None else v.clone(memory_format=torch.contiguous_format) for r, v in views.items() if r in inputs}
    contig.update({r: None for r in outputs})
    log.take()
    want = call(contig)
    log_contig = log.take()
    got = call(views)
    log_views = log.take()
    torch.cuda.synchronize()
    case = (row["id"], assignment)
    assert "?" not in log_contig and "?overflow" not in log_contig, log_contig
    missing = kc.missing_from_log(row, log_contig)
    assert not missing, (case, missing, sorted({kc.key_str(kc.parse_symbol(s)) for s in log_contig}))
    assert log_views == log_contig, (case, "a layout changed the dispatch", log_contig, log_views)
    for role in outputs:   # the call wrote into the views it was given
        assert got[role].data_ptr() == views[role].data_ptr() and got[role].stride() == views[role].stride(), (case, role)
    for name in want:
        assert _same(got[name], want[name]), (case, name, "differs from the contiguous call",
                                              float((got[name].float() - want[name].float()).abs().nan_to_num(nan=float("inf")).max()))
    for a in arenas:
        if a.kind == "output":
            assert a.outside_intact(), (case, "a store outside an output view")
        elif any(v.data_ptr() == views[r].data_ptr() for r in inout for v in a.views):
            assert a.outside_unchanged(), (case, "a store outside the rows of the appended cache")
        else:
            assert a.unchanged(), (case, "an input arena was written")
    for name in list(outputs) + list(inout):
        assert not torch.isnan(got[name].float()).any(), (case, name)
        w = want[name].float()
        assert torch.isfinite(w).all() and float(w.max()) > float(w.min()), (case, name, "the contiguous result is finite and not constant")
    return want, got


def _mask(row):
    mode = row["mode"]
    window = tuple(row.get("window") or (kc.WINDOW if mode == "local" else (-1, -1)))
    if mode != "local":
        window = (-1, -1)
    return mode == "causal", window


# ---- fa_fwd / fa_varlen_fwd / fa_bwd / fa_varlen_bwd (also the (192, 128) pair) ------------------------------------------------------------------
def _case_attn(log, row, assignment):
    be = log.be
    dtype = DT[row["dt"]]
    d, dv = (192, 128) if row["kind"] == "dv" else (row["d"], row["d"])
    causal, (wl, wr) = _mask(row)
    cap, pd = row.get("cap", 0.0), row.get("pd", 0.0)
    seed = zlib.crc32(row["id"].encode())
    g = torch.Generator().manual_seed(seed)
    varlen, run_bwd = row.get("varlen", False), any(k[0].startswith("fa_bwd") for k in row["keys"])
    payload = pd > 0 and not row.get("replay", False)   # (the 64-per-wave dropout variant has no random-byte output: asking for it would change the dispatch)
    slopes = (torch.rand(H, generator=g) * 0.5 + 0.05).to(DEV) if row.get("alibi") else None
    if varlen:
        lq, lk = (row["lens"], row["lens"]) if row.get("lens") else ([row["sq"], 120], [row["sk"], 150])
        cu = lambda ls: torch.tensor([0] + [sum(ls[:i + 1]) for i in range(len(ls))], dtype=torch.int32, device=DEV)
        cu_q, cu_k = cu(lq), cu(lk)
        sq_, sk_ = (sum(lq),), (sum(lk),)
    else:
        sq_, sk_ = (B, row["sq"]), (B, row["sk"])
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype).to(DEV)
    inputs = dict(q=rnd(*sq_, H, d), k=rnd(*sk_, HK, d), v=rnd(*sk_, HK, dv))
    outputs = dict(out=(*sq_, H, dv))
    if run_bwd:
        inputs["dout"] = rnd(*sq_, H, dv)
        outputs.update(dq=(*sq_, H, d), dk=(*sk_, HK, d), dv=(*sk_, HK, dv))
    scale = d ** -0.5

    def call(t):
        torch.manual_seed(seed)   # dropout: both calls draw from the same generator state
        if varlen:
            out, lse, p, rng = be.varlen_fwd(t["q"], t["k"], t["v"], t["out"], cu_q, cu_k, None, None, None, slopes, max(lq), max(lk), pd, scale, False, causal, wl, wr, cap,
                                             payload, None)
        else:
            out, lse, p, rng = be.fwd(t["q"], t["k"], t["v"], t["out"], slopes, pd, scale, causal, wl, wr, cap, payload, None)
        res = dict(out=out, lse=lse)
        if payload:
            res["p"] = p
        if run_bwd:
            if varlen:
                grads = be.varlen_bwd(t["dout"], t["q"], t["k"], t["v"], out, lse, t["dq"], t["dk"], t["dv"], cu_q, cu_k, slopes, max(lq), max(lk), pd, scale, False, causal, wl, wr,
                                      cap, False, None, rng)
            else:
                grads = be.bwd(t["dout"], t["q"], t["k"], t["v"], out, lse, t["dq"], t["dk"], t["dv"], slopes, pd, scale, causal, wl, wr, cap, False, None, rng)
            res.update(dq=grads[0], dk=grads[1], dv=grads[2], softmax_d=grads[3])
            res["sched"] = torch.tensor([be.last_schedule()["bwd_list"]])
        return res

    want, _ = _execute(log, row, assignment, inputs, outputs, call, dtype)
    if row.get("lens"):
        assert int(want["sched"]) == 1, "the uneven packed batch runs the backward through its work lists"
    elif varlen and run_bwd:
        assert int(want["sched"]) == 0


# ---- fa_fwd_kvcache: split keys + combine, paged prefill, MLA, the fp8 cache ----------------------------------------------------------------------
def _census_paged(kL, vL, g):
    from tests.test_kernel_census_gpu import _paged
    return _paged(kL, vL, 256, g)


def _case_kvcache(log, row, assignment):
    be = log.be
    dtype, d = DT[row["dt"]], row["d"]
    g = torch.Generator().manual_seed(zlib.crc32(row["id"].encode()))
    q = torch.randn(B, row["sq"], H, d, generator=g).to(dtype)
    bc = B + 2 if row.get("batch_idx") else B
    kL, vL = torch.randn(bc, row["cap"], HK, d, generator=g).to(dtype), torch.randn(bc, row["cap"], HK, d, generator=g).to(dtype)
    kc_, vc_, table = _census_paged(kL, vL, g) if row["paged"] else (kL, vL, None)
    idx = torch.tensor([3, 1], dtype=torch.int32, device=DEV) if row.get("batch_idx") else None
    lens = torch.tensor(row["lens"], dtype=torch.int32, device=DEV)
    table = None if table is None else table.to(DEV)
    wl, wr = row["window"]

    def call(t):
        out, lse = be.fwd_kvcache(t["q"], t["kcache"], t["vcache"], None, None, lens, None, None, idx, None, table, None, t["out"], d ** -0.5, row["causal"], wl, wr, 0.0, True,
                                  row["splits"])
        assert (be.last_schedule()["fwd_splits"] > 1) == (row["splits"] > 1)
        if "nopack" in row["id"]:
            assert be.last_schedule()["fwd_pack"] == 1
        return dict(out=out, lse=lse)

    _execute(log, row, assignment, dict(q=q.to(DEV), kcache=kc_.to(DEV), vcache=vc_.to(DEV)), dict(out=tuple(q.shape)), call, dtype, paged=row["paged"])


def _case_mla(log, row, assignment):
    from tests import test_mla_decode_gpu as m
    be = log.be
    dtype = DT[row["dt"]]
    g = torch.Generator().manual_seed(zlib.crc32(row["id"].encode()))
    causal, (wl, wr) = _mask(row)
    q = torch.randn(B, row["sq"], H, m.D, generator=g).to(dtype)
    kL = torch.randn(B, row["cap"], HK, m.D, generator=g).to(dtype)
    kcache, idx, bt = m._layout(row["layout"], kL, list(row["lens"]), g)
    lens = torch.tensor(row["lens"], dtype=torch.int32, device=DEV)
    bt = None if bt is None else bt.to(DEV)

    def call(t):   # the layout is the cache's as a whole: v stays the latent view of k
        out, lse = be.fwd_kvcache(t["q"], t["kcache"], t["kcache"][..., :m.DV], None, None, lens, None, None, idx, None, bt, None, t["out"], m.SCALE, causal, wl, wr, 0.0, True,
                                  row["splits"])
        m._assert_mla(dtype, H // HK, row["splits"])
        return dict(out=out, lse=lse)

    _execute(log, row, assignment, dict(q=q.to(DEV), kcache=kcache.contiguous()), dict(out=(B, row["sq"], H, m.DV)), call, dtype, paged=bt is not None)


def _case_fp8(log, row, assignment):
    from tests import test_fwd_fp8_gpu as m
    be = log.be
    g = torch.Generator().manual_seed(zlib.crc32(row["id"].encode()))
    d = row["d"]
    causal, (wl, wr) = _mask(row)
    q, k, v = m._fp8((B, row["sq"], H, d), g, 2.0), m._fp8((B, row["sk"], HK, d), g, 2.0), m._fp8((B, row["sk"], HK, d), g)
    qd, kd, vd = m._descales("rand", B, HK, g)

    def call(t):
        out, lse = be.fwd_fp8(t["q"], t["k"], t["v"], t["out"], qd, kd, vd, d ** -0.5, causal, wl, wr)
        return dict(out=out, lse=lse)

    _execute(log, row, assignment, dict(q=q.to(DEV), k=k.to(DEV), v=v.to(DEV)), dict(out=(B, row["sq"], H, d)), call, torch.bfloat16)


def _case_fp8kv(log, row, assignment):
    from tests import test_kvcache_fp8_gpu as m
    be = log.be
    g = torch.Generator().manual_seed(zlib.crc32(row["id"].encode()))
    d, lens = row["d"], list(row["lens"])
    causal, (wl, wr) = _mask(row)
    q = m._fp8((B, row["sq"], H, d), g, 2.0)
    kL, vL = m._fp8((B, row["cap"], HK, d), g, 2.0), m._fp8((B, row["cap"], HK, d), g)
    kcache, vcache, idx, bt = m._layout(row["layout"], kL, vL, lens, g)
    qd, kd, vd = m._descales("rand", B, HK, g)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    idx, bt = (None if x is None else x.to(DEV) for x in (idx, bt))

    def call(t):
        out, lse = be.fwd_kvcache_fp8(t["q"], t["kcache"], t["vcache"], None, None, lens_t, idx, bt, t["out"], qd, kd, vd, d ** -0.5, causal, wl, wr, row["splits"])
        return dict(out=out, lse=lse)

    _execute(log, row, assignment, dict(q=q.to(DEV), kcache=kcache.to(DEV), vcache=vcache.to(DEV)), dict(out=(B, row["sq"], H, d)), call, torch.bfloat16, paged=bt is not None)


# ---- append, rotary -------------------------------------------------------------------------------------------------------------------------------
def _case_append(log, row, assignment):
    """New rows into a paged cache (shuffled table, the rows straddle a page edge) and into a batch-indexed one.  The caches are read and written: their views must equal
    the contiguous call's caches, and every row of the arena outside them -- with the views' own rows outside [len, len + S_new) covered by that equality -- stays bit-identical."""
    be = log.be
    d, s_new, dtype = 128, 37, torch.bfloat16
    lens = torch.tensor([240, 3], dtype=torch.int32, device=DEV)
    for paged in (True, False):
        g = torch.Generator().manual_seed(11 + paged)
        rnd = lambda *s: torch.randn(*s, generator=g).to(dtype)
        q, kn, vn = rnd(B, s_new, H, d), rnd(B, s_new, HK, d), rnd(B, s_new, HK, d)
        kL, vL = rnd(B, 512, HK, d), rnd(B, 512, HK, d)
        kp, vp, table = _census_paged(kL, vL, g) if paged else (kL, vL, None)
        idx = None if paged else torch.tensor([1, 0], dtype=torch.int32, device=DEV)
        table = None if table is None else table.to(DEV)

        def call(t):
            out, lse = be.fwd_kvcache(t["q"], t["kcache"], t["vcache"], t["knew"], t["vnew"], lens, None, None, idx, None, table, None, t["out"], d ** -0.5, True, -1, -1, 0.0, True, 0)
            return dict(out=out, lse=lse, kcache=t["kcache"], vcache=t["vcache"])

        before = kp.to(DEV)
        want, _ = _execute(log, row, assignment, dict(q=q.to(DEV), kcache=before, vcache=vp.to(DEV), knew=kn.to(DEV), vnew=vn.to(DEV)), dict(out=tuple(q.shape)), call, dtype,
                           paged=paged, inout=("kcache", "vcache"))
        changed = (_bits(want["kcache"]) != _bits(before)).flatten(2).any(-1)   # (entry or page, row): exactly the S_new appended rows of each entry
        assert int(changed.sum()) == B * s_new, (paged, int(changed.sum()))


def _rotary_into(log, x, y, cos, sin, offsets, interleaved, per_token):
    """backend._rotary with the output tensor given (the binder allocates its own)."""
    import ctypes as C
    be, cabi = log.be, log.cabi
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device) if y is None else y
    r = cabi.FaRotaryParams()
    r.x, r.y, r.cos, r.sin, r.seqlen_offsets = be._ptr(x), be._ptr(y), be._ptr(cos), be._ptr(sin), be._ptr(offsets)
    r.x_batch_stride, r.x_row_stride, r.x_head_stride = x.stride(0), x.stride(1), x.stride(2)
    r.y_batch_stride, r.y_row_stride, r.y_head_stride = y.stride(0), y.stride(1), y.stride(2)
    r.cos_row_stride = cos.stride(0)
    r.b, r.s, r.h, r.d = x.shape
    r.rotary_dim, r.seqlen_ro = 2 * cos.shape[1], cos.shape[0]
    r.interleaved, r.per_token, r.dtype = int(interleaved), int(per_token), be._dtype_code(x)
    cabi.check(cabi.load().fa_rotary(C.byref(r), C.c_void_p(be._stream_ptr(x.device))))
    return y


def _case_rotary(log, row, assignment):
    dtype = DT[row["dt"]]
    torch.manual_seed(5)
    S, d, rd = 37, 128, 64
    x = torch.randn(B, S, H, d, device=DEV, dtype=dtype)
    ang = torch.rand(128, rd // 2, device=DEV) * 2 * math.pi
    cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
    offsets = torch.tensor([3, 90], dtype=torch.int32, device=DEV)

    def call(t):
        res = {}
        for interleaved in (False, True):
            for per_token in (True, False):
                y = _rotary_into(log, t["q"], t["out"], cos, sin, offsets, interleaved, per_token)
                res[f"y-{interleaved}-{per_token}"] = y.clone()
        res["out"] = y
        return res

    _execute(log, row, assignment, dict(q=x), dict(out=tuple(x.shape)), call, dtype)


_CASE = {"attn": _case_attn, "dv": _case_attn, "kvcache": _case_kvcache, "mla": _case_mla, "fp8": _case_fp8, "fp8kv": _case_fp8kv, "append": _case_append, "rotary": _case_rotary}


@pytest.mark.parametrize("row,assignment", CASES, ids=[f"{r['id']}-{a}" for r, a in CASES])
def test_layout_matrix(knobs, monkeypatch, row, assignment):
    _CASE[row["kind"]](_Log(knobs, monkeypatch, row["knobs"]), row, assignment)


# ---- through autograd, default dispatch ------------------------------------------------------------------------------------------------------------
def _leaf(x):
    return x.detach().clone().requires_grad_()


def test_autograd_flash_attn_func_on_a_bhsd_leaf():
    from flash_attn_amd.flash_attn_interface import flash_attn_func
    torch.manual_seed(21)
    mk = lambda s, h: torch.randn(B, h, s, 128, device=DEV, dtype=torch.bfloat16)
    leaves = [_leaf(mk(165, H)), _leaf(mk(203, HK)), _leaf(mk(203, HK))]   # (B, H, S, D) leaves, seen through transpose(1, 2)
    dense = [_leaf(t.transpose(1, 2).contiguous()) for t in leaves]
    do = torch.randn(B, H, 165, 128, device=DEV, dtype=torch.bfloat16).transpose(1, 2)
    out = flash_attn_func(*[t.transpose(1, 2) for t in leaves], causal=True)
    ref = flash_attn_func(*dense, causal=True)
    assert _same(out, ref)
    out.backward(do)
    ref.backward(do.contiguous())
    for t, r in zip(leaves, dense):
        assert t.grad.shape == t.shape and t.grad.stride() == t.stride(), "the gradient lands in the leaf's own layout"
        assert _same(t.grad.transpose(1, 2), r.grad) and torch.isfinite(r.grad.float()).all() and float(r.grad.float().abs().max()) > 0


def test_autograd_flash_attn_func_on_slices_of_one_fused_leaf():
    from flash_attn_amd.flash_attn_interface import flash_attn_func
    torch.manual_seed(22)
    S, d = 165, 128
    qkv = _leaf(torch.randn(B, S, (H + 2 * HK) * d, device=DEV, dtype=torch.bfloat16))   # one fused projection output
    cut = lambda t: [x.unflatten(-1, (-1, d)) for x in t.split([H * d, HK * d, HK * d], dim=-1)]
    dense = [_leaf(x.contiguous()) for x in cut(qkv.detach())]
    do = torch.randn(B, S, H, d, device=DEV, dtype=torch.bfloat16)
    out, ref = flash_attn_func(*cut(qkv), causal=True), flash_attn_func(*dense, causal=True)
    assert _same(out, ref)
    out.backward(do)
    ref.backward(do)
    assert qkv.grad.shape == qkv.shape and qkv.grad.is_contiguous()
    for got, r in zip(cut(qkv.grad), dense):
        assert _same(got, r.grad) and float(r.grad.float().abs().max()) > 0


def test_autograd_flash_attn_varlen_func_on_a_transposed_packed_leaf():
    from flash_attn_amd.flash_attn_interface import flash_attn_varlen_func
    torch.manual_seed(23)
    lens, d = [165, 120], 128
    cu = torch.tensor([0, 165, 285], dtype=torch.int32, device=DEV)
    leaves = [_leaf(torch.randn(h, sum(lens), d, device=DEV, dtype=torch.bfloat16)) for h in (H, HK, HK)]   # (H, T, D) leaves, seen through transpose(0, 1)
    dense = [_leaf(t.transpose(0, 1).contiguous()) for t in leaves]
    do = torch.randn(sum(lens), H, d, device=DEV, dtype=torch.bfloat16)
    out = flash_attn_varlen_func(*[t.transpose(0, 1) for t in leaves], cu, cu, max(lens), max(lens), causal=True)
    ref = flash_attn_varlen_func(*dense, cu, cu, max(lens), max(lens), causal=True)
    assert _same(out, ref)
    out.backward(do)
    ref.backward(do)
    for t, r in zip(leaves, dense):
        assert t.grad.shape == t.shape and t.grad.stride() == t.stride()
        assert _same(t.grad.transpose(0, 1), r.grad) and float(r.grad.float().abs().max()) > 0


def test_flash_attn_with_kvcache_decode_q_slice_and_strided_out():
    from flash_attn_amd.flash_attn_interface import flash_attn_with_kvcache
    torch.manual_seed(24)
    d, cap = 128, 700
    qkv = torch.randn(B, 1, (H + 2 * HK) * d, device=DEV, dtype=torch.bfloat16)   # the decode step's fused projection: q, and the new k / v rows
    q, kn, vn = (x.unflatten(-1, (-1, d)) for x in qkv.split([H * d, HK * d, HK * d], dim=-1))
    kc_, vc_ = (torch.randn(B, cap, HK, d, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    lens = torch.tensor([650, 389], dtype=torch.int32, device=DEV)
    arena, out = L.place("padded_head", shape=(B, 1, H, d), dtype=torch.bfloat16, kind="output", device=DEV)
    k1, v1, k2, v2 = kc_.clone(), vc_.clone(), kc_.clone(), vc_.clone()
    got = flash_attn_with_kvcache(q, k1, v1, k=kn, v=vn, cache_seqlens=lens, causal=True, out=out)
    ref = flash_attn_with_kvcache(q.contiguous(), k2, v2, k=kn.contiguous(), v=vn.contiguous(), cache_seqlens=lens, causal=True)
    assert got.data_ptr() == out.data_ptr() and _same(got, ref) and arena.outside_intact()
    assert _same(k1, k2) and _same(v1, v2) and not _same(k1, kc_)
    assert torch.isfinite(ref.float()).all() and float(ref.float().max()) > float(ref.float().min())


# ---- the alignment contract through the binder ------------------------------------------------------------------------------------------------------
def test_misaligned_view_is_refused_before_anything_is_enqueued(knobs, monkeypatch):
    """x[..., 4:4 + D] of a wider buffer: a base 8 bytes off the 16-byte chunks every kernel moves.  The C ABI refuses it by name on the host; the launch log of the
    refused call is empty.  (Nothing misaligned ever reaches the device.)"""
    log = _Log(knobs, monkeypatch, {})
    be = log.be
    d = 64
    wide = lambda s, h: torch.randn(B, s, h, d + 8, device=DEV, dtype=torch.bfloat16)
    q, k, v = wide(165, H)[..., :d], wide(203, HK)[..., :d], wide(203, HK)[..., :d]
    for name in ("q", "k", "v"):
        t = dict(q=q, k=k, v=v)
        t[name] = wide(*((165, H) if name == "q" else (203, HK)))[..., 4:4 + d]
        assert t[name].data_ptr() % 16 == 8
        with pytest.raises(RuntimeError, match=rf"fa_fwd: {name} must be 16-byte aligned"):
            be.fwd(t["q"], t["k"], t["v"], None, None, 0.0, d ** -0.5, True, -1, -1, 0.0, False, None)
        assert be.launch_log() == [] and log.take() == []
    odd = torch.randn(B, 203, HK * (d + 4), device=DEV, dtype=torch.bfloat16).unflatten(-1, (HK, d + 4))[..., :d]   # heads D + 4 apart
    with pytest.raises(RuntimeError, match="head stride of k"):
        be.fwd(q, odd, v, None, None, 0.0, d ** -0.5, True, -1, -1, 0.0, False, None)
    assert be.launch_log() == []
    out, lse, _, _ = be.fwd(q, k, v, None, None, 0.0, d ** -0.5, True, -1, -1, 0.0, False, None)   # the aligned views of the same buffers run
    assert len(be.launch_log()) >= 1 and torch.isfinite(out.float()).all()
