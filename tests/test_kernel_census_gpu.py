"""Every compiled kernel instantiation, once, against the oracle (tests/_kernel_census.py RECIPES; the CPU half proves that the table claims every kernel
of the library).  Each case sets the row's knobs plus FA_DEBUG_LAUNCH_LOG=1 and FA_DEBUG_POISON_WS=1, runs the row's call at the smallest shape that still
exercises the kernel, asserts that the library's launch log holds every key the row claims -- a recipe that silently falls back to a sibling
instantiation fails there -- and compares every result tensor under the rule its path already has:

  fa_fwd / fa_varlen_fwd and their backward    tools/fuzz_gpu.py run_case: 2x (out) / 3x (gradients) the same-dtype PyTorch error + one input ulp (+ the delta term of dq / dk)
  LSE                                          lse_tolerance() of tests/test_baseline_configs_gpu.py, +inf exactly on the rows that see no key
  KV cache (split keys, paged 64-per-wave)     the bounds of tests/test_kvcache_gpu.py
  fp8, fp8 KV cache, (192, 128), MLA decode    the check functions of their modules
  rotary / append / work list / rng state      the _rotary_ref bound / bit-exact cache / bit-exact against FA_VARLEN_LIST=0 / a seeded dropout call that reproduces

The library is driven through the ctypes binder on the calling thread (the launch log and the workspace poison are per thread / a binder feature); the backward of a
public function is therefore run by calling the autograd node's own backward instead of handing it to the autograd engine's worker thread.
With FA_CENSUS_REPORT=<file> every case appends its id, its worst error / tolerance and its keys there (profiles/kernel_census.txt)."""
import math
import os
import sys
import zlib

import numpy as np
import pytest
import torch

from tests import _kernel_census as kc
from tests._util import attention_torch, max_abs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
B, H, HK = 2, 4, 2
DEV = "cuda"


class _Census:
    """The launch log of everything a case runs: the ctypes binder checks every launching C call's return code with _cabi.check, which here reads the log first."""

    def __init__(self, knobs, monkeypatch, row):
        from flash_attn_amd import _cabi, backend, flash_attn_interface as fi
        self.knobs, self.row, self.names, self.be = knobs, row, [], backend
        for name, value in dict(row["knobs"], FA_DEBUG_LAUNCH_LOG=1, FA_DEBUG_POISON_WS=1).items():
            knobs.set(name, value)
        check = _cabi.check

        def logged_check(rc):
            self.names.extend(backend.launch_log())
            return check(rc)
        monkeypatch.setattr(_cabi, "check", logged_check)
        monkeypatch.setattr(fi, "flash_attn_gpu", backend)

    def assert_reached(self):
        assert "?" not in self.names and "?overflow" not in self.names, self.names
        missing = kc.missing_from_log(self.row, self.names)
        assert not missing, (self.row["id"], missing, sorted({kc.key_str(kc.parse_symbol(s)) for s in self.names}))

    def report(self, ratio):
        print(f"census {self.row['id']}: worst error / tolerance {ratio:.3f}")
        path = os.environ.get("FA_CENSUS_REPORT")
        if path:
            with open(path, "a") as f:
                f.write("%s %.4f %s\n" % (self.row["id"], ratio, " ".join(kc.key_str(k) for k in self.row["keys"])))


@pytest.fixture
def census(knobs, monkeypatch, request):
    return _Census(knobs, monkeypatch, request.param)


def _lse_ratio(lse, ref, tol):
    """LSE against the oracle: +inf exactly where the oracle has it, the rest within tol; returns error / tolerance."""
    lse = lse.detach().float().cpu().numpy().astype(np.float64)
    fin = np.isfinite(ref)
    assert lse.shape == ref.shape and (np.isposinf(lse) == ~fin).all(), "LSE is +inf exactly on the rows that see no key"
    err = float(np.abs(lse[fin] - ref[fin]).max()) if fin.any() else 0.0
    print(f"  lse err {err:.3e} tol {tol:.3e}")
    assert err < tol, (err, tol)
    return err / tol


# ---- fa_fwd / fa_varlen_fwd + backward ---------------------------------------------------------------------------------------------------------
def _run_attn(c):
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_gpu
    from oracle import attention_oracle as orc
    from tests.test_baseline_configs_gpu import lse_tolerance
    r = c.row
    case = dict(n=zlib.crc32(r["id"].encode()) % 100000 + 1, dtype=DT[r["dt"]], d=r["d"], h=H, hk=HK, B=B, sq=r["sq"], sk=r["sk"], mode=r["mode"], window=r["window"],
                alibi=r["alibi"], cap=r["cap"], pd=r["pd"], varlen=r["varlen"], lq=[r["sq"], 120], lk=[r["sk"], 150])
    seen = {}

    def call(fn, *a, **kw):
        mask = None
        if r["replay"]:
            # dropout on a kernel without the random-byte output: the keep mask is a function of (seed, offset, position) alone, so the same call on the lock-step
            # kernel, from the same generator state, returns the bytes this call's kernel draws
            state = torch.cuda.get_rng_state()
            c.knobs.set("FA_FWD_NW", 8)
            mask = fn(*a, **kw)[2]
            torch.cuda.set_rng_state(state)
            c.knobs.set("FA_FWD_NW", r["knobs"]["FA_FWD_NW"])
            kw = {k: v for k, v in kw.items() if k != "return_attn_probs"}
        res = fn(*a, **kw)
        seen.update(sched=c.be.last_schedule(), args=a, kw=kw, out=res[0] if isinstance(res, tuple) else res)
        return (res, None, mask) if r["replay"] else res

    def grad(out, inputs, g):   # the node's own backward, on this thread
        node = out.grad_fn
        return node._forward_cls.backward(node, g)[:3]

    worst, failures = {}, []
    fuzz_gpu.run_case(case, worst, failures, call=call, grad=grad)
    assert not failures, failures
    c.assert_reached()
    # LSE: what the forward saved for its backward
    a, kw, out = seen["args"], seen["kw"], seen["out"]
    lse = out.grad_fn.saved_tensors[4]
    alibi = kw.get("alibi_slopes")
    common = (None, kw["causal"], kw["window_size"], kw.get("softcap", 0.0), None if alibi is None else alibi.cpu().numpy())
    if r["varlen"]:
        _, ref = orc.varlen_fwd(a[0], a[1], a[2], a[3], a[4], *common)
    else:
        _, ref = orc.attention_fwd(a[0], a[1], a[2], *common)
    fin = np.isfinite(ref)
    tol = lse_tolerance(seen["sched"], case["dtype"], float(np.abs(ref[fin]).max()) if fin.any() else 0.0)
    c.report(max(max(worst.values()), _lse_ratio(lse, ref, tol)))


# ---- fa_fwd_kvcache: split keys + combine, paged cache on the 64-rows-per-wave kernel ----------------------------------------------------------
def _paged(kL, vL, page, g):
    """The logical caches (B, cap, Hk, D) cut into pages in shuffled order, three pages never referenced."""
    Bc, cap = kL.shape[:2]
    per = cap // page
    nb = Bc * per + 3
    table = torch.randperm(nb, generator=g)[:Bc * per].reshape(Bc, per)
    kp, vp = torch.randn(nb, page, *kL.shape[2:], generator=g).to(kL.dtype), torch.randn(nb, page, *vL.shape[2:], generator=g).to(vL.dtype)
    for b in range(Bc):
        for j in range(per):
            kp[table[b, j]], vp[table[b, j]] = kL[b, j * page:(j + 1) * page], vL[b, j * page:(j + 1) * page]
    return kp, vp, table.to(torch.int32)


def _run_kvcache(c):
    from tests.test_baseline_configs_gpu import lse_tolerance
    from tests.test_kvcache_gpu import _oracle
    r = c.row
    dtype, d = DT[r["dt"]], r["d"]
    g = torch.Generator().manual_seed(zlib.crc32(r["id"].encode()))
    q = torch.randn(B, r["sq"], H, d, generator=g).to(dtype)
    kL, vL = torch.randn(B, r["cap"], HK, d, generator=g).to(dtype), torch.randn(B, r["cap"], HK, d, generator=g).to(dtype)
    kc_, vc_, table = _paged(kL, vL, 256, g) if r["paged"] else (kL, vL, None)
    lens = torch.tensor(r["lens"], dtype=torch.int32)
    dv = lambda t: None if t is None else t.to(DEV)
    out, lse = c.be.fwd_kvcache(dv(q), dv(kc_), dv(vc_), None, None, dv(lens), None, None, None, None, dv(table), None, None, d ** -0.5, r["causal"], r["window"][0],
                                r["window"][1], 0.0, True, r["splits"])
    sched = c.be.last_schedule()
    c.assert_reached()
    assert (sched["fwd_splits"] > 1) == (r["splits"] > 1), sched
    o_ref, l_ref = _oracle(q, kL, vL, r["lens"], r["causal"], r["window"])
    # (tests/test_kvcache_gpu.py: 2e-2 on a bf16 out, 5e-3 on an fp16 one)
    tol_o = 2e-2 if dtype == torch.bfloat16 else 5e-3
    err_o = max_abs(out.float().cpu(), torch.from_numpy(o_ref))
    print(f"  out err {err_o:.3e} tol {tol_o:.3e}")
    assert err_o < tol_o
    fin = np.isfinite(l_ref)
    c.report(max(err_o / tol_o, _lse_ratio(lse, l_ref, lse_tolerance(sched, dtype, float(np.abs(l_ref[fin]).max())))))


# ---- absorbed MLA decode ------------------------------------------------------------------------------------------------------------------------
def _run_mla(c):
    from tests import test_mla_decode_gpu as m
    r = c.row
    dtype = DT[r["dt"]]
    g = torch.Generator().manual_seed(zlib.crc32(r["id"].encode()))
    causal, window = r["mode"] == "causal", kc.WINDOW if r["mode"] == "local" else (-1, -1)
    q = torch.randn(B, r["sq"], H, m.D, generator=g).to(dtype)
    kL = torch.randn(B, r["cap"], HK, m.D, generator=g).to(dtype)
    kcache, idx, bt = m._layout(r["layout"], kL, list(r["lens"]), g)
    out, lse = m._call(c.be, q, kcache, torch.tensor(r["lens"], dtype=torch.int32), idx, bt, causal, window, r["splits"])
    m._assert_mla(dtype, H // HK, r["splits"])
    c.assert_reached()
    o32, l32, base = torch.zeros(B, r["sq"], H, m.DV), torch.full((B, H, r["sq"]), float("inf")), 0.0
    for b, L in enumerate(r["lens"]):   # the references of the module's _problem: fp32 and same-dtype PyTorch per entry
        qb, kb = q[b:b + 1].to(DEV), kL[b:b + 1, :L].to(DEV)
        o, l = attention_torch(qb.float(), kb.float(), kb[..., :m.DV].float(), causal, window, m.SCALE, True)
        opt, _ = attention_torch(qb, kb, kb[..., :m.DV], causal, window, m.SCALE, False)
        o32[b], l32[b] = o[0].cpu(), l[0].cpu()
        base = max(base, max_abs(opt.float(), o))
    m._check(out, lse, (None, None, o32, l32, base), r["id"])
    c.report(max_abs(out.float().cpu(), o32) / (2 * base + 1e-4))


# ---- q / k head dim 192, v / o head dim 128 ----------------------------------------------------------------------------------------------------------
def _run_dv(c):
    from tests import test_headdim_v_gpu as m
    r = c.row
    dtype = DT[r["dt"]]
    torch.manual_seed(zlib.crc32(r["id"].encode()))
    causal, window = r["mode"] == "causal", kc.WINDOW if r["mode"] == "local" else (-1, -1)
    q = torch.randn(B, r["sq"], H, m.D, device=DEV, dtype=dtype)
    k = torch.randn(B, r["sk"], HK, m.D, device=DEV, dtype=dtype)
    v = torch.randn(B, r["sk"], HK, m.DV, device=DEV, dtype=dtype)
    do = torch.randn(B, r["sq"], H, m.DV, device=DEV, dtype=dtype)
    out, lse = m._fwd(c.be, q, k, v, causal, window)
    grads = m._bwd(c.be, do, q, k, v, out, lse, causal, window)
    c.assert_reached()
    m._check(out, lse, grads, q, k, v, do, causal, window, r["id"])   # (asserts and prints its figures; it returns none)
    c.report(float("nan"))


# ---- fp8 forward, fp8 KV cache -------------------------------------------------------------------------------------------------------------------
def _run_fp8(c):
    from tests import test_fwd_fp8_gpu as m
    r = c.row
    g = torch.Generator().manual_seed(zlib.crc32(r["id"].encode()))
    d = r["d"]
    causal, window = r["mode"] == "causal", kc.WINDOW if r["mode"] == "local" else (-1, -1)
    q, k, v = m._fp8((B, r["sq"], H, d), g, 2.0), m._fp8((B, r["sk"], HK, d), g, 2.0), m._fp8((B, r["sk"], HK, d), g)
    ds = m._descales("rand", B, HK, g)
    out, lse = m._run(q, k, v, ds, d ** -0.5, causal, window)
    c.assert_reached()
    _, err_l = m._check_parity(q, k, v, ds, d ** -0.5, causal, window, out, lse)
    c.report(err_l / 5e-4)   # (out is bounded element by element inside the check; its LSE bound is 5e-4 relative)


def _run_fp8kv(c):
    from tests import test_kvcache_fp8_gpu as m
    r = c.row
    g = torch.Generator().manual_seed(zlib.crc32(r["id"].encode()))
    d, lens = r["d"], list(r["lens"])
    causal, window = r["mode"] == "causal", kc.WINDOW if r["mode"] == "local" else (-1, -1)
    q = m._fp8((B, r["sq"], H, d), g, 2.0)
    kL, vL = m._fp8((B, r["cap"], HK, d), g, 2.0), m._fp8((B, r["cap"], HK, d), g)
    kcache, vcache, idx, bt = m._layout(r["layout"], kL, vL, lens, g)
    ds = m._descales("rand", B, HK, g)
    out, lse = m._call(c.be, q, kcache.to(DEV), vcache.to(DEV), None, None, torch.tensor(lens, dtype=torch.int32), idx, bt, ds, d ** -0.5, causal, window, r["splits"])
    c.assert_reached()
    err_l = max(m._check_entry(q[b:b + 1], kL[b:b + 1, :lens[b]], vL[b:b + 1, :lens[b]], tuple(t[b:b + 1] for t in ds), d ** -0.5, causal, window, out[b:b + 1],
                               lse[b:b + 1])[1] for b in range(B))
    c.report(err_l / 5e-4)   # (as the fp8 forward)


# ---- the small kernels ---------------------------------------------------------------------------------------------------------------------------
def _run_rotary(c):
    from flash_attn_amd import _cabi
    from tests.test_kvcache_gpu import _rotary_ref
    dtype = DT[c.row["dt"]]
    torch.manual_seed(5)
    S, d, rd = 37, 128, 64
    x = torch.randn(B, S, H, d, device=DEV, dtype=dtype)
    ang = torch.rand(128, rd // 2, device=DEV) * 2 * math.pi
    cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
    offsets = torch.tensor([3, 90], dtype=torch.int32, device=DEV)
    worst = 0.0
    for interleaved in (False, True):
        for per_token in (True, False):
            y = c.be._rotary(_cabi.load(), x, cos, sin, offsets, interleaved, per_token)
            ref = _rotary_ref(x, cos, sin, offsets.cpu(), interleaved, per_token)
            e = max_abs(y.float().cpu(), ref.float())
            assert e < 4e-2, (interleaved, per_token, e)   # (tests/test_kvcache_gpu.py test_kvcache_rotary: one bf16 ulp of |x| <= 4)
            assert torch.equal(y[..., rd:], x[..., rd:])   # the channels behind rotary_dim are copied
            worst = max(worst, e / 4e-2)
    c.assert_reached()
    c.report(worst)


def _run_append(c):
    """New rows into a paged cache (shuffled table, the rows straddle a page edge) and into a batch-indexed one: the cache holds exactly the new rows there and its old
    contents everywhere else, bit for bit."""
    g = torch.Generator().manual_seed(11)
    d, page, s_new, dtype = 128, 256, 37, torch.bfloat16
    raw = lambda t: t.view(torch.int16)
    q = torch.randn(B, s_new, H, d, generator=g).to(dtype)
    kn, vn = torch.randn(B, s_new, HK, d, generator=g).to(dtype), torch.randn(B, s_new, HK, d, generator=g).to(dtype)
    lens = [240, 3]
    for paged in (True, False):
        kL, vL = torch.randn(B, 512, HK, d, generator=g).to(dtype), torch.randn(B, 512, HK, d, generator=g).to(dtype)
        kp, vp, table = _paged(kL, vL, page, g) if paged else (kL, vL, None)
        idx = None if paged else torch.tensor([1, 0], dtype=torch.int32)
        want_k, want_v = kp.clone(), vp.clone()
        for b in range(B):
            for t in range(s_new):
                row = lens[b] + t
                at = (int(table[b, row // page]), row % page) if paged else (int(idx[b]), row)
                want_k[at], want_v[at] = kn[b, t], vn[b, t]
        kd, vd = kp.to(DEV), vp.to(DEV)
        dv = lambda t: None if t is None else t.to(DEV)
        c.be.fwd_kvcache(dv(q), kd, vd, dv(kn), dv(vn), torch.tensor(lens, dtype=torch.int32, device=DEV), None, None, dv(idx), None, dv(table), None, None, d ** -0.5, True,
                         -1, -1, 0.0, True, 0)
        assert torch.equal(raw(kd.cpu()), raw(want_k)) and torch.equal(raw(vd.cpu()), raw(want_v)), paged
    c.assert_reached()
    c.report(0.0)


def _run_schedule(c):
    """A packed batch uneven enough for the work list (one 512-row sequence among fifteen of 37 rows: 64 dense blocks of 128 rows against 24 listed): the call with
    the list equals the call on the dense grid bit for bit."""
    torch.manual_seed(13)
    lens = [37] * 7 + [512] + [37] * 8
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)
    q = torch.randn(sum(lens), H, 64, device=DEV, dtype=torch.bfloat16)
    k, v = torch.randn(sum(lens), HK, 64, device=DEV, dtype=torch.bfloat16), torch.randn(sum(lens), HK, 64, device=DEV, dtype=torch.bfloat16)
    run = lambda: c.be.varlen_fwd(q, k, v, None, cu, cu, None, None, None, None, max(lens), max(lens), 0.0, 0.125, False, True, -1, -1, 0.0, False, None)[:2]
    out, lse = run()
    assert c.be.last_schedule()["fwd_list"] == 1
    c.assert_reached()
    c.knobs.set("FA_VARLEN_LIST", 0)
    out0, lse0 = run()
    assert c.be.last_schedule()["fwd_list"] == 0
    assert torch.equal(out.view(torch.int16), out0.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse0.view(torch.int32))
    c.report(0.0)


def _run_set_rng(c):
    """The kernel writes (seed, offset) of the default generator to the device; a dropout call seeded the same way draws the same mask, another seed another one."""
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(1234)
    gen = torch.cuda.default_generators[dev.index]
    off = gen.get_offset()
    state = c.be._new_rng_state(dev, 0.1, B, H)
    c.assert_reached()
    assert state.cpu().tolist() == [1234, off] and gen.get_offset() > off
    q = torch.randn(B, 165, H, 64, device=DEV, dtype=torch.bfloat16)
    k, v = torch.randn(B, 203, HK, 64, device=DEV, dtype=torch.bfloat16), torch.randn(B, 203, HK, 64, device=DEV, dtype=torch.bfloat16)

    def run(seed):
        torch.manual_seed(seed)
        return c.be.fwd(q, k, v, None, None, 0.25, 0.125, True, -1, -1, 0.0, True, None)
    a, b_, other = run(7), run(7), run(8)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[2], b_[2]) and torch.equal(a[3], b_[3])
    assert not torch.equal(a[2], other[2]) and not torch.equal(a[0], other[0])
    c.report(0.0)


_RUN = {"attn": _run_attn, "kvcache": _run_kvcache, "mla": _run_mla, "dv": _run_dv, "fp8": _run_fp8, "fp8kv": _run_fp8kv, "rotary": _run_rotary, "append": _run_append,
        "schedule": _run_schedule, "set_rng": _run_set_rng}


@pytest.mark.parametrize("census", kc.RECIPES, ids=[r["id"] for r in kc.RECIPES], indirect=True)
def test_census(census):
    _RUN[census.row["kind"]](census)
