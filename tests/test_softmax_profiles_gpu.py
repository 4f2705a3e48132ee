"""The online-softmax rescale paths of every forward kernel, forced on purpose.  On randn data the deferred rescale (FwdK::rescale_thr) runs once per row, at the first
key; here tests/_softmax_profiles.py builds inputs whose scores follow a prescribed profile -- `fire` keys that exceed the row's maximum by the threshold + 2, `hold` keys
just under it, growths in two consecutive 32-key steps, stairs of +6, masked decoys beside a visible fire -- at key 0, at the first and last key of a tile, at Sk - 1
inside the partial last tile, on a wave's causal diagonal, at a window's first key, at the first and last key of a KV split and behind cache_seqlens[b].  The builder
asserts its conditions on the fp64 scores before anything runs; tests/test_softmax_profiles_cpu.py shows that a stand-in with any of nine rescale mistakes is reported
on the same case lists (sp.case_lists()).

Every test pins one kernel by knobs, asserts through backend.last_schedule() that it ran, and judges every case against oracle.attention_oracle in fp64 by the rule its
family already has (sp.out_tolerance: none is changed here; the e4m3 families go through their modules' own check functions).  LSE: +inf exactly where the oracle has
it, elsewhere sp.LSE_BOUND -- 2 x the stand-in's worst deviation on these lists, never below 2e-3, set once from the CPU run (profiles/softmax_profiles.txt).
Cross checks: the default threshold against FA_RESCALE_THR=0 (output rounding), fp16 at FA_RESCALE_THR=16 against 15 (bit for bit: the host's cap), and the rows WITHOUT
a target against a call whose targets are removed (bit for bit: the cold path is exact for a factor of 1).  Last, the backward on the same rows.

Dropout is out of scope (the keep mask would have to be replayed for every profile).  With FA_SOFTMAX_PROFILES_REPORT=<file> the cases and the worst error / bound per
family are appended there."""
import os

import numpy as np
import pytest
import torch

from tests import _softmax_profiles as sp

pytestmark = pytest.mark.gpu
DEV = "cuda"
LISTS = sp.case_lists()
DTYPES = ["bf16", "fp16"]
_BOOK = {}   # {family label: [cases, worst out / bound, worst lse / bound, placements]}
_MINE = {}   # the same, of the test that is running (need() reads this one)


@pytest.fixture(scope="module")
def be():
    from flash_attn_amd import backend
    return backend


@pytest.fixture(autouse=True)
def _own_book():
    _MINE.clear()
    yield


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("FA_SOFTMAX_PROFILES_REPORT")
    if path and _BOOK:
        with open(path, "a") as f:
            f.write("# tests/test_softmax_profiles_gpu.py: %d cases\n# %-44s cases  out/bound  lse/bound  placements\n" % (sum(v[0] for v in _BOOK.values()), "kernel"))
            for label, (n, r_o, r_l, places) in sorted(_BOOK.items()):
                f.write("%-46s %5d  %9.3f  %9.3f  %s\n" % (label, n, r_o, r_l, ",".join(sorted(places))))


def label_of(s):
    """The kernel that ran, from the schedule: its name without the dtype and the template tail, plus what the call added."""
    name = s["name"].replace("fa::", "").replace("<bf16,", "<T,").replace("<f16,", "<T,")
    return name + (" +splitkv" if s["fwd_splits"] > 1 else "") + (" packed-rows" if s["fwd_pack"] > 1 else "") + (" list" if s["fwd_list"] else "")


FWD_KERNEL = {4: ("fa_fwd_kernel<T,%d,", ",4,feat0,lockstep"), 8: ("fa_fwd_kernel<T,%d,", ",8,feat0,lockstep"), 16: ("fa_fwd_kernel<T,%d,", "pingpong"),
              34: ("fa_fwd_il_kernel<T,%d,4,", ""), 38: ("fa_fwd_il_kernel<T,%d,8,", ""), 64: ("fa_fwd_w64_kernel<T,%d", "")}


def assert_kernel(be, d, nw, extra=""):
    s = be.last_schedule()
    label = label_of(s)
    a, b = FWD_KERNEL[nw]
    assert (a % d) in label and b in label and extra in label, (nw, d, extra, label)
    return label


def book(label, p, r_o, r_l, problems, what):
    for b in (_BOOK, _MINE):
        e = b.setdefault(label, [0, 0.0, 0.0, set()])
        e[0] += 1
        e[1], e[2] = max(e[1], r_o), max(e[2], r_l)
        e[3] |= set(sp.placements_of(p.plan))
    print("%s | %s: out error / bound %.3f, lse error / bound %.3f" % (label, what, r_o, r_l))
    assert not problems, (label, what, problems)


def need(*fragments):
    """The kernels the RUNNING test pinned have booked cases in it, with at least three distinct target placements (first / interior / last tile, the mask edges where
    there are masks)."""
    for frag in fragments:
        hits = {l: v for l, v in _MINE.items() if frag in l}
        assert hits, (frag, sorted(_MINE))
        assert len(set().union(*(v[3] for v in hits.values()))) >= 3, (frag, hits)


def on_dev(p, t):
    return t.to(device=DEV, dtype=sp.DT[p.dtype])


def slopes_of(p):
    return None if p.slopes is None else torch.tensor(p.slopes, dtype=torch.float32, device=DEV)


def fwd(be, p):
    """The fixed-length forward on one profile (B = 1) -> out (Sq, H, Dv), lse (H, Sq)."""
    out, lse = be.fwd(on_dev(p, p.q)[None], on_dev(p, p.k[:p.sk])[None], on_dev(p, p.v[:p.sk])[None], None, slopes_of(p), 0.0, sp.SCALE, bool(p.mask[0]), p.mask[1], p.mask[2],
                      p.softcap, False, None)[:2]
    return out[0], lse[0]


def what_of(p, extra=""):
    return "%s d%d/%d Sq %d Sk %d mask %s thr %s%s" % (p.dtype, p.d, p.dv, p.sq, p.sk, p.mask, p.thr, extra)


def judged(label, family, spec, out, lse, extra=""):
    p, o, l, err_pt = sp.reference(spec)
    r_o, r_l, problems = sp.judge(out, lse, o, l, sp.out_tolerance(family, p, o, err_pt))
    book(label, p, r_o, r_l, problems, what_of(p, extra))


def spacing(x, dtype):
    """The distance between neighbouring values of the dtype at |x| (elementwise, fp64)."""
    bits = 7 if dtype == "bf16" else 10
    return torch.exp2(torch.floor(torch.log2(x.abs().double().clamp(min=2.0 ** -14))) - bits)


def assert_output_rounding(a, b, lse_a, lse_b, p, what):
    """Two thresholds on the same inputs: each run rounds P once to the dtype (2^-(bits + 2) relative) before the product with V, |v| <= 4 here, so the fp32
    results differ by at most 2 x 2^-(bits + 2) x 4; each is then rounded to the dtype: one spacing more.  LSE: fp32 sums of the same terms, 1e-4 (tests/test_fwd_gpu.py)."""
    bits = 7 if p.dtype == "bf16" else 10
    tol = spacing(torch.maximum(a.abs(), b.abs()), p.dtype) + 2 * 2.0 ** -(bits + 2) * 4
    diff = (a.double() - b.double()).abs()
    assert bool((diff <= tol).all()), (what, float(diff.max()), float((diff / tol).max()))
    fin = torch.isfinite(lse_a)
    assert torch.equal(fin, torch.isfinite(lse_b)) and float((lse_a[fin] - lse_b[fin]).abs().max()) < 1e-4, what


def same_bits(a, b):
    raw = lambda x: x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)
    return torch.equal(raw(a), raw(b))


def untouched_rows(p):
    keep = torch.ones(p.sq, p.h, dtype=torch.bool)
    for t in p.targets:
        keep[t[1], t[2]] = False
    return keep.to(DEV)


# ---------------------------------------------------------------- forward schedules ----------------------------------------------------------------
@pytest.mark.parametrize("thr", [8, 0])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("nw", [4, 8, 16, 34, 38, 64])
def test_forward_schedules(be, knobs, nw, d, dt, thr):
    """Every forward schedule, no mask / causal with Sq != Sk / a two-sided window, at the default threshold ((600, 1100)) and at FA_RESCALE_THR=0 ((160, 333)).  The
    default-threshold cases run once more at threshold 0 (the two agree to output rounding) and once with the targets removed (the rows without a target agree bit for bit)."""
    knobs.set("FA_FWD_NW", nw)
    for spec in LISTS["fwd %s d%d thr%d" % (dt, d, thr)]:
        p = sp.profile_of(spec)
        knobs.set("FA_RESCALE_THR", thr) if thr == 0 else knobs.unset("FA_RESCALE_THR")
        out, lse = fwd(be, p)
        label = assert_kernel(be, d, nw)
        judged(label, "fwd", spec, out, lse)
        if thr == 8:
            knobs.set("FA_RESCALE_THR", 0)
            out0, lse0 = fwd(be, p)
            assert_output_rounding(out, out0, lse, lse0, p, what_of(p, " default threshold against 0"))
            knobs.unset("FA_RESCALE_THR")
            bare = sp.profile_of(spec, targets=False)
            out_b, lse_b = fwd(be, bare)
            keep = untouched_rows(p)
            assert same_bits(out[keep], out_b[keep]) and same_bits(lse.t()[keep], lse_b.t()[keep]), (label, what_of(p), "rows without a target differ from the call without targets")
            assert not same_bits(out[~keep], out_b[~keep])
    need(FWD_KERNEL[nw][0] % d)


@pytest.mark.parametrize("nw", [4, 8, 16, 34, 38, 64])
def test_fp16_threshold_cap(be, knobs, nw):
    """fp16: the host caps the threshold at 15 so that P stays below 65504.  FA_RESCALE_THR=16 equals =15 bit for bit, and the rows of the stairs (+6 in each of four
    steps: 24 in all) are finite."""
    knobs.set("FA_FWD_NW", nw)
    for spec in LISTS["fwd fp16 thr15"]:
        p = sp.profile_of(spec)
        knobs.set("FA_RESCALE_THR", 15)
        out, lse = fwd(be, p)
        label = assert_kernel(be, p.d, nw)
        judged(label, "fwd", spec, out, lse, " FA_RESCALE_THR=15")
        knobs.set("FA_RESCALE_THR", 16)
        out16, lse16 = fwd(be, p)
        assert same_bits(out, out16) and same_bits(lse, lse16), (label, "FA_RESCALE_THR=16 is not the capped 15")
        stairs = [(t[1], t[2]) for t in p.targets if t[0] == "stairs"]
        assert stairs and all(bool(torch.isfinite(out[r, h].float()).all()) for r, h in stairs)
    need(FWD_KERNEL[nw][0] % 64, FWD_KERNEL[nw][0] % 128)


@pytest.mark.parametrize("dt", DTYPES)
def test_lockstep_head_dims_and_packed_rows(be, knobs, dt):
    """Head dim 256, 96 (trimmed) and 40 (run-time column bound) on the lock-step kernel, and its packed-GQA layout (fwd_pack > 1: Sq = 16 rows of four heads in one block)."""
    for spec in LISTS["lockstep dims %s" % dt]:
        p = sp.profile_of(spec)
        out, lse = fwd(be, p)
        label = label_of(be.last_schedule())
        assert "fa_fwd_kernel<T,%d,4," % {256: 256, 96: 96, 40: 64}[p.d] in label, label
        judged("d%d " % p.d + label, "fwd", spec, out, lse)
    knobs.set("FA_PACK_GQA", 1)
    for spec in LISTS["packed gqa %s" % dt]:
        p = sp.profile_of(spec)
        out, lse = fwd(be, p)
        s = be.last_schedule()
        assert s["fwd_pack"] == 4 and "fa_fwd_kernel<T,128," in label_of(s), s
        judged(label_of(s), "fwd", spec, out, lse)
    need("fa_fwd_kernel<T,256,4,", "fa_fwd_kernel<T,96,4,", "d40 fa_fwd_kernel<T,64,4,", "packed-rows")


# ---------------------------------------------------------------- the 64-rows-per-wave kernel ----------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("feat", ["alibi", "softcap"])
def test_w64_alibi_and_softcap(be, knobs, feat, dt):
    """Causal ALiBi (the bias rides in the C operand that rescale() re-bases) and softcap (capoff under a forced growth).  A capped score cannot exceed
    softcap * log2(e) = 34.6 log2 units at sp.SOFTCAP = 24: every height, the decoys' included, stays under it -- the builder asserts that."""
    knobs.set("FA_FWD_NW", 64)
    for spec in LISTS["w64 %s %s" % (feat, dt)]:
        p = sp.profile_of(spec)
        out, lse = fwd(be, p)
        label = assert_kernel(be, p.d, 64, feat)
        judged(label, "fwd", spec, out, lse)
        bare = sp.profile_of(spec, targets=False)
        out_b, lse_b = fwd(be, bare)
        keep = untouched_rows(p)
        assert same_bits(out[keep], out_b[keep]) and same_bits(lse.t()[keep], lse_b.t()[keep]), (label, what_of(p), "rows without a target differ from the call without targets")
    need(feat)


PERSIST_B, PERSIST_PAIRS = 2, 36   # 2 x 72 heads x 2 blocks of 256 rows = 288 blocks for the chip's 256 CUs: a second, partial round of the persistent walk


def traced_w64_grids(tmp_path, dt, shapes):
    """tools/w64_grid_probe.py under `rocprofv3 --kernel-trace`, in a process of its own: [Grid_Size_X // Workgroup_Size_X] of the 64-rows-per-wave dispatches, in launch
    order -- per shape the FA_W64_PERSIST=1 launch, then the =0 one.  (last_schedule() does not say whether a launch was persistent; the dispatch's grid does.)"""
    import csv
    import glob
    import shutil
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FA_") or k == "FA_GFX950_LIB"}
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(tmp_path), "--", sys.executable, os.path.join(root, "tools", "w64_grid_probe.py"), dt] +
                       [",".join(str(int(x)) for x in sh) for sh in shapes], capture_output=True, text=True, timeout=120, env=env)
    files = glob.glob(os.path.join(str(tmp_path), "**", "*kernel_trace.csv"), recursive=True)
    assert r.returncode == 0 and len(files) == 1, (r.returncode, r.stdout[-1500:], r.stderr[-1500:], files)
    with open(files[0]) as f:
        rows = sorted((int(x["Dispatch_Id"]), int(x["Grid_Size_X"]) // int(x["Workgroup_Size_X"])) for x in csv.DictReader(f) if "fa_fwd_w64_kernel" in x["Kernel_Name"])
    return [g for _, g in rows]


@pytest.mark.parametrize("dt", DTYPES)
def test_w64_persistent_on_and_off(be, knobs, tmp_path, dt):
    """The persistent walk under a forced rescale: m / l / the pending factor are set up again for every block a workgroup walks.  The profile ((512, 1100): two blocks
    of 256 rows) is replicated over 2 batch entries x 36 head pairs -- 288 blocks for 256 CUs, so 32 blocks, spiked rows among them, are reached in a second round
    (mirrored inside its units under the causal mask).  That FA_W64_PERSIST=1 launches one workgroup per CU at these shapes and =0 one per block is read from a kernel
    trace of the same launches on random data (the grid depends on the shape, the mask and the knob alone); both runs are judged, and they agree bit for bit."""
    specs = LISTS["w64 persist %s" % dt]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = PERSIST_B * PERSIST_PAIRS * 2 * 2
    assert blocks > cus, "the shape no longer exceeds the chip: no second round"
    grids = traced_w64_grids(tmp_path, dt, [(PERSIST_B, sp.profile_of(s).sq, sp.profile_of(s).sk, 2 * PERSIST_PAIRS, PERSIST_PAIRS, sp.profile_of(s).d, sp.profile_of(s).mask[0])
                                            for s in specs])
    assert grids == [cus // 8 * 8, blocks] * len(specs), (grids, cus, blocks)
    knobs.set("FA_FWD_NW", 64)
    for spec in specs:
        p, o_ref, l_ref, err_pt = sp.reference(spec)
        q = on_dev(p, p.q.repeat(1, PERSIST_PAIRS, 1))[None].expand(PERSIST_B, -1, -1, -1).contiguous()
        k = on_dev(p, p.k[:p.sk].repeat(1, PERSIST_PAIRS, 1))[None].expand(PERSIST_B, -1, -1, -1).contiguous()
        v = on_dev(p, p.v[:p.sk].repeat(1, PERSIST_PAIRS, 1))[None].expand(PERSIST_B, -1, -1, -1).contiguous()
        runs = {}
        for persist in (1, 0):
            knobs.set("FA_W64_PERSIST", persist)
            out, lse = be.fwd(q, k, v, None, None, 0.0, sp.SCALE, bool(p.mask[0]), p.mask[1], p.mask[2], 0.0, False, None)[:2]
            label = assert_kernel(be, p.d, 64) + " persist=%d" % persist
            runs[persist] = (out, lse)
            # every replica of the profile, (batch entry, head pair): the worst one is judged
            o5 = out.reshape(PERSIST_B, p.sq, PERSIST_PAIRS, 2, p.dv)
            l5 = lse.reshape(PERSIST_B, PERSIST_PAIRS, 2, p.sq)
            assert bool(torch.isfinite(o5.float()).all())
            e_o = (o5.double() - o_ref.to(DEV)[None, :, None]).abs().amax(dim=(1, 3, 4))                      # (B, pairs)
            e_l = torch.nan_to_num((l5.double() - l_ref.to(DEV)[None, None]).abs(), nan=0.0, posinf=0.0).amax(dim=(2, 3))
            for idx in {int(e_o.argmax()), int(e_l.argmax())}:
                b_, j = divmod(idx, PERSIST_PAIRS)
                judged(label, "fwd", spec, o5[b_, :, j], l5[b_, j], " replica (%d, %d) of %d blocks" % (b_, j, blocks))
        assert same_bits(runs[1][0], runs[0][0]) and same_bits(runs[1][1], runs[0][1]), (what_of(p), "the persistent walk and the one-workgroup-per-block grid differ")
    need("persist=1", "persist=0")


FILLERS = 40   # short sequences around the profile's: 41 entries x 3 blocks of 256 rows is a dense grid of 123 slots against 44 listed (fa_api.cpp varlen_list_entries)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("work_list", [1, 0])
def test_w64_packed_batches(be, knobs, work_list, dt):
    """The profile as entry 20 of a packed batch of 41 (the others: 8 quiet rows against 40 keys), with the work list and with FA_VARLEN_LIST=0."""
    knobs.set("FA_FWD_NW", 64)
    knobs.set("FA_VARLEN_LIST", work_list)
    g = torch.Generator().manual_seed(5)
    for spec in [LISTS["fwd %s d%d thr8" % (dt, d)][i] for d, i in ((128, 1), (128, 2), (64, 1))]:
        p = sp.profile_of(spec)
        lens_q, lens_k = [8] * FILLERS, [40] * FILLERS
        lens_q.insert(20, p.sq), lens_k.insert(20, p.sk)
        cu_q = torch.tensor([0] + list(np.cumsum(lens_q)), dtype=torch.int32, device=DEV)
        cu_k = torch.tensor([0] + list(np.cumsum(lens_k)), dtype=torch.int32, device=DEV)
        q = (torch.randn(sum(lens_q), p.h, p.d, generator=g) * 0.3).to(sp.DT[dt])
        k, v = (torch.randn(sum(lens_k), p.hk, p.d, generator=g) * 0.3).to(sp.DT[dt]), torch.randn(sum(lens_k), p.hk, p.d, generator=g).to(sp.DT[dt])
        q0, k0 = int(cu_q[20]), int(cu_k[20])
        q[q0:q0 + p.sq], k[k0:k0 + p.sk], v[k0:k0 + p.sk] = p.q.to(sp.DT[dt]), p.k[:p.sk].to(sp.DT[dt]), p.v[:p.sk].to(sp.DT[dt])
        out, lse = be.varlen_fwd(q.to(DEV), k.to(DEV), v.to(DEV), None, cu_q, cu_k, None, None, None, None, max(lens_q), max(lens_k), 0.0, sp.SCALE, False, bool(p.mask[0]),
                                 p.mask[1], p.mask[2], 0.0, False, None)[:2]
        s = be.last_schedule()
        assert s["fwd_list"] == work_list, s
        assert bool(torch.isfinite(out.float()).all())
        judged(assert_kernel(be, p.d, 64) + " varlen", "fwd", spec, out[q0:q0 + p.sq], lse[:, q0:q0 + p.sq])
    need(" list varlen" if work_list else "> varlen")


@pytest.mark.parametrize("dt", DTYPES)
def test_w64_paged_prefill(be, knobs, dt):
    """The keys behind a shuffled page table (256 rows a page), NaN behind the sequence's end."""
    knobs.set("FA_FWD_NW", 64)
    for spec in [LISTS["fwd %s d%d thr8" % (dt, d)][i] for d, i in ((128, 1), (128, 2), (64, 0))]:
        p = sp.profile_of(spec)
        page, per = 256, -(-p.sk // 256)
        table = torch.randperm(per + 2, generator=torch.Generator().manual_seed(3))[:per].reshape(1, per).to(torch.int32)
        kl = torch.full((per * page, p.hk, p.d), float("nan"))
        vl = kl.clone()
        kl[:p.sk], vl[:p.sk] = p.k[:p.sk], p.v[:p.sk]
        kp = torch.full((per + 2, page, p.hk, p.d), float("nan"))
        vp = kp.clone()
        kp[table.long().reshape(-1)], vp[table.long().reshape(-1)] = kl.reshape(per, page, p.hk, p.d), vl.reshape(per, page, p.hk, p.d)
        cu_q, cu_k = (torch.tensor([0, n], dtype=torch.int32, device=DEV) for n in (p.sq, p.sk))
        out, lse = be.varlen_fwd(on_dev(p, p.q), on_dev(p, kp), on_dev(p, vp), None, cu_q, cu_k, None, None, table.to(DEV), None, p.sq, p.sk, 0.0, sp.SCALE, False,
                                 bool(p.mask[0]), p.mask[1], p.mask[2], 0.0, False, None)[:2]
        judged(assert_kernel(be, p.d, 64, "paged") + " varlen", "fwd", spec, out, lse)
    need("paged")


# ---------------------------------------------------------------- q / k 192, v / o 128 ----------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_v_head_dim_128_beside_192(be, knobs, dt):
    for spec in LISTS["dv %s" % dt]:
        p = sp.profile_of(spec)
        knobs.set("FA_RESCALE_THR", 0) if p.thr == 0 else knobs.unset("FA_RESCALE_THR")
        out, lse = fwd(be, p)
        label = label_of(be.last_schedule())
        assert "fa_fwd_dv_kernel<T,192,128" in label, label
        judged(label, "dv", spec, out, lse)
    need("fa_fwd_dv_kernel")


# ---------------------------------------------------------------- KV cache, MLA decode ----------------------------------------------------------------
def cache_of(profs, paged, dtype, latent=False, seed=0):
    """The logical caches (B, CACHE_CAP, Hk, D): an entry's keys, the row behind its length (the decoy), then quiet random rows; paged: 256-row pages in shuffled order.
    -> (k cache, v cache, block table) on the CPU, in `dtype`."""
    g = torch.Generator().manual_seed(17 + seed)
    p0 = profs[0]
    n = len(profs)
    kl = torch.randn(n, sp.CACHE_CAP, p0.hk, p0.d, generator=g) * 0.2
    vl = torch.randn(n, sp.CACHE_CAP, p0.hk, p0.dv, generator=g)
    for b, p in enumerate(profs):
        kl[b, :p.sk + p.extra], vl[b, :p.sk + p.extra] = p.k, p.v
    table = None
    if paged:                                                    # (assembled in fp32, converted once: the profiles' values are exact in the dtype)
        per = sp.CACHE_CAP // 256
        table = torch.randperm(n * per + 2, generator=g)[:n * per].reshape(n, per)
        kp, vp = torch.zeros(n * per + 2, 256, p0.hk, p0.d), torch.zeros(n * per + 2, 256, p0.hk, p0.dv)
        kp[table.reshape(-1)], vp[table.reshape(-1)] = kl.reshape(n * per, 256, p0.hk, p0.d), vl.reshape(n * per, 256, p0.hk, p0.dv)
        kl, vl, table = kp, vp, table.to(torch.int32)
    kl = kl.to(dtype)
    return kl, (kl[..., :p0.dv] if latent else vl.to(dtype)), table


def run_cache(be, specs, splits, paged, latent=False):
    profs = [sp.profile_of(s) for s in specs]
    p0 = profs[0]
    dtype = sp.DT[p0.dtype]
    kc, vc, table = cache_of(profs, paged, dtype, latent)
    kc = kc.to(DEV)
    vc = kc[..., :p0.dv] if latent else vc.to(DEV)
    q = torch.stack([p.q for p in profs]).to(device=DEV, dtype=dtype)
    lens = torch.tensor([p.sk for p in profs], dtype=torch.int32, device=DEV)
    out, lse = be.fwd_kvcache(q, kc, vc, None, None, lens, None, None, None, None, None if table is None else table.to(DEV), None, None, sp.SCALE, bool(p0.mask[0]), -1, -1, 0.0,
                              True, splits)
    s = be.last_schedule()
    assert s["fwd_splits"] == splits, s   # (sp.split_edges() places the targets for exactly this many ranges)
    return profs, out, lse, s


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged256"])
@pytest.mark.parametrize("splits", [1, 2, 3, 4])
def test_kvcache_and_its_split_merge(be, knobs, splits, paged, dt):
    """fwd_kvcache with cache_seqlens (1100, 300) in a cache of 1536 rows: the fire sits on the first key of the last split that holds keys, a hold on the key before it, the
    other splits hold background only (their partial maxima lie more than 10 log2 units below), the short entry leaves the later splits empty, and a decoy waits behind
    cache_seqlens[0]."""
    for sq in (1, 4):
        specs = LISTS["kvcache %s sq%d splits%d" % (dt, sq, splits)]
        profs, out, lse, s = run_cache(be, specs, splits, paged)
        label = label_of(s) + " kvcache" + (" paged" if paged else "")
        assert "fa_fwd_kernel<T,128," in label, label
        if splits > 1:
            edges = sp.split_edges(splits)
            fire = [t for t in profs[0].targets if t[0] == "fire" and t[3] in edges and t[3] > 0]
            assert fire and profs[1].sk <= edges[1] * (splits - 1), "one split holds the fire; the short entry leaves the last split empty"
        for b, spec in enumerate(specs):
            judged(label, "kvcache", spec, out[b], lse[b], " entry %d splits %d" % (b, splits))
    need(" kvcache", "+splitkv" if splits > 1 else " kvcache")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("splits", [1, 3])
def test_mla_decode(be, knobs, splits, dt):
    """The absorbed MLA pair (q / k 576, v / o 512 = k_cache[..., :512]), H = 16, Sq 1 and 2: the target channels lie in 512 .. 575, the rope part, so that V stays clean."""
    for sq in (1, 2):
        specs = LISTS["mla %s sq%d splits%d" % (dt, sq, splits)]
        for paged in (False, True):
            profs, out, lse, s = run_cache(be, specs, splits, paged, latent=True)
            assert s["fwd_kernel"] == 7 and s["d"] == 576 and s["dv"] == 512 and s["fwd_pack"] == 16, s
            for b, spec in enumerate(specs):
                judged(label_of(s) + (" paged" if paged else ""), "mla", spec, out[b], lse[b], " entry %d splits %d" % (b, splits))
    need("fa_fwd_mla_kernel")


# ---------------------------------------------------------------- e4m3 ----------------------------------------------------------------
@pytest.mark.parametrize("thr", [8, 0])
@pytest.mark.parametrize("d", [64, 128])
def test_fp8_forward(be, knobs, d, thr):
    """P is rounded to e4m3 (448 is the largest finite value, there is no inf): the host caps the threshold at 8.  A `fire` exceeds m by more than that, moves m and gets
    P = 1; the largest P of these profiles is the `hold`'s, 2^7 (e4m3 holds k to one part in 16, so no key can be put exactly on the cap, where P = 2^8).  Judged by the
    module's own _check_parity, which also asserts that out is finite (a NaN means P left e4m3's range)."""
    from tests import test_fwd_fp8_gpu as m
    knobs.set("FA_RESCALE_THR", 0) if thr == 0 else knobs.unset("FA_RESCALE_THR")
    for spec in LISTS["fp8 d%d thr%d" % (d, thr)]:
        p = sp.profile_of(spec)
        q, k, v = (t.to(m.FP8)[None] for t in (p.q, p.k[:p.sk], p.v[:p.sk]))
        out, lse = m._run(q, k, v, (None, None, None), sp.SCALE, bool(p.mask[0]), p.mask[1:])
        s = be.last_schedule()
        assert s["fwd_kernel"] == 4, s
        err_o, err_l = m._check_parity(q, k, v, (None, None, None), sp.SCALE, bool(p.mask[0]), p.mask[1:], out, lse)
        book(label_of(s), p, float("nan"), err_l / 5e-4, [], what_of(p))
    need("fp8")


@pytest.mark.parametrize("thr", [8, 0])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged256"])
def test_fp8_kvcache_decode(be, knobs, paged, thr):
    from tests import test_kvcache_fp8_gpu as m
    knobs.set("FA_RESCALE_THR", 0) if thr == 0 else knobs.unset("FA_RESCALE_THR")
    for sq in (1, 4):
        specs = LISTS["fp8 kvcache sq%d%s" % (sq, "" if thr else " thr0")]
        profs = [sp.profile_of(s) for s in specs]
        kc, vc, table = cache_of(profs, paged, m.FP8)
        q = torch.stack([p.q for p in profs]).to(m.FP8)
        lens = torch.tensor([p.sk for p in profs], dtype=torch.int32)
        causal = bool(profs[0].mask[0])
        out, lse = m._call(be, q, kc.to(DEV), vc.to(DEV), None, None, lens, None, table, (None, None, None), sp.SCALE, causal, (-1, -1), 1)
        s = be.last_schedule()
        assert s["fwd_kernel"] == 5, s
        for b, p in enumerate(profs):
            _, err_l = m._check_entry(q[b:b + 1], p.k[None, :p.sk].to(m.FP8), p.v[None, :p.sk].to(m.FP8), (None, None, None), sp.SCALE, causal, (-1, -1), out[b:b + 1], lse[b:b + 1])
            book(label_of(s) + (" paged" if paged else ""), p, float("nan"), err_l / 5e-4, [], what_of(p, " entry %d" % b))
    need("fp8_kv")


# ---------------------------------------------------------------- the backward on the same rows ----------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mode", ["default", "fused", "w64pair"])
def test_backward_on_the_spiked_rows(be, knobs, mode, dt):
    """The backward recomputes P from the forward's LSE: the causal (600, 1100) case and its window twin through the default dispatch, FA_BWD_MODE=3 and the pinned
    64-per-wave pair, against attention_bwd under the reference's 3x rule (tests/_util.py matrix_bound's form, the baseline computed on these inputs).  The fused launch
    accepts no left window bound, so under FA_BWD_MODE=3 only the causal case is a fused run; the window twin is asserted to fall back to the pair and booked as such."""
    from oracle import attention_oracle as orc
    if mode == "fused":
        knobs.set("FA_BWD_MODE", 3)
    if mode == "w64pair":
        knobs.set("FA_BWD_MODE", -1), knobs.set("FA_BWD_DQ_NW", 64), knobs.set("FA_BWD_DKDV", 64)
    for spec in LISTS["fwd %s d128 thr8" % dt][1:]:
        p = sp.profile_of(spec)
        causal, win = bool(p.mask[0]), p.mask[1:]
        q, k, v = on_dev(p, p.q)[None], on_dev(p, p.k[:p.sk])[None], on_dev(p, p.v[:p.sk])[None]
        dout = torch.randn(p.sq, p.h, p.dv, generator=torch.Generator().manual_seed(23)).to(sp.DT[dt])
        out, lse = be.fwd(q, k, v, None, None, 0.0, sp.SCALE, causal, win[0], win[1], 0.0, False, None)[:2]
        grads = be.bwd(dout.to(DEV)[None], q, k, v, out, lse, None, None, None, None, 0.0, sp.SCALE, causal, win[0], win[1], 0.0, False, None, None)[:3]
        s = be.last_schedule()
        if mode == "fused":   # (the fused launch takes no left window bound: the window twin is NOT a fused run, it must fall back to the recomputing pair)
            assert s["bwd_spill"] == (3 if causal else 0), s
        if mode == "w64pair":
            assert s["bwd_dq_nw"] == 64 and s["bwd_dkdv_nw"] == 64 and s["bwd_spill"] == 0, s
        ref = orc.attention_bwd(dout[None], p.q[None], p.k[None, :p.sk], p.v[None, :p.sk], None, None, sp.SCALE, causal, win)[:3]
        base = sp.baseline(p, DEV, dout)[1:]
        label = "bwd d128 dq_nw=%d dkdv_nw=%d spill=%d (%s)" % (s["bwd_dq_nw"], s["bwd_dkdv_nw"], s["bwd_spill"], "fused refused: the pair" if mode == "fused" and not causal else mode)
        worst, problems = 0.0, []
        for nm, got, r, b_ in zip(("dq", "dk", "dv"), grads, ref, base):
            r = torch.from_numpy(np.asarray(r))[0]
            e, e_pt = float((got[0].double().cpu() - r).abs().max()), float((b_.double() - r).abs().max())
            tol = 3 * e_pt + 1e-4
            print("%s %s err %.3e (pytorch %.3e)" % (label, nm, e, e_pt))
            worst = max(worst, e / tol)
            if not (e <= tol and bool(torch.isfinite(got.float()).all())):
                problems.append("%s error %.3e above %.3e" % (nm, e, tol))
        book(label, p, worst, 0.0, problems, what_of(p))
    need("bwd d128")
