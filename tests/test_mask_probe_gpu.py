"""Is the visible set of every attention kernel EXACTLY right?  The parity tests judge a mask by an error bound, which cannot see one key too many or too few at
a window edge (one key in 500 moves out by 1/500, below the bf16 rounding the bound allows).  Here q = 0 makes P exactly uniform over a row's visible keys and
coded V / dO / K turn every output element into a count of at most 16 terms (tests/_mask_probe.py: the construction, the cap, the 0.25 threshold); the expected
sets are the oracle's normalize_window + visible_mask -- for packed batches normalised by max_seqlen_k, for the cache path built from each entry's own
cache_seqlens[b] (+ S_new).  tests/test_mask_probe_cpu.py shows that the probe reports every wrong mask of its list.

Each test pins one kernel (FA_* knobs through the `knobs` fixture, FA_BWD_GSPLIT included: conftest.py does not list this module) and loops over shapes x masks
x dtypes on tiny tensors; after every call backend.last_schedule() names what ran, the case is booked to THAT kernel, and the pinned kernel must end with at
least 20 probed cases.  With FA_MASK_PROBE_MARGINS=<file> the worst normalised deviation per kernel, dtype and decoder is written there
(profiles/mask_probe_margins.txt is such a run).

Out of scope: the fp8 forward and the fp8 KV cache (their P is rounded to e4m3, which cannot hold 1 / n for counts above 4: they keep their one-hot tests),
and ALiBi and dropout (P is not uniform under either)."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from tests import _mask_probe as mp

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
DN = {torch.bfloat16: "bf16", torch.float16: "fp16"}
_BOOK = {}      # {kernel label: cases}
_MARGINS = {}   # {(kernel label, dtype name): {decoder: worst deviation}}


@pytest.fixture(scope="module")
def be():
    from flash_attn_amd import backend
    return backend


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    yield
    for fn in (fwd_exp, rand_k):   # the expected sets and codes live on the device: give the memory back to the rest of the session
        fn.cache_clear()
    mp.clear_caches()
    torch.cuda.empty_cache()
    path = os.environ.get("FA_MASK_PROBE_MARGINS")
    if path and _MARGINS:
        with open(path, "w") as f:
            f.write("# worst normalised deviation of each decoder of the mask probe (tests/test_mask_probe_gpu.py, tests/_mask_probe.py) per kernel and dtype; threshold 0.25,\n"
                    "# at most 16 terms per element.  count = |exp(lse) - n|, fine / coarse = |out n - count| of the two V codes, dv = |dV - fp64|, dq = |n dQ / scale - fp64|\n"
                    "# kernel                                                              dtype  cases   " + "".join("%9s" % d for d in ("count", "fine", "coarse", "dv", "dq")) + "\n")
            for (label, dn), m in sorted(_MARGINS.items()):
                f.write("%-70s %-5s %6d   " % (label, dn, m["cases"]) + "".join(("%9.4f" % m[d]) if d in m else "%9s" % "-" for d in ("count", "fine", "coarse", "dv", "dq")) + "\n")


def fwd_label(s, d):
    """The call's head dim goes first: head dim 40 runs the kernel built for 64 and must not be booked with the calls at 64."""
    name = s["name"].replace("<bf16,", "<T,").replace("<f16,", "<T,")
    return "fwd d%d " % d + name + (" +splitkv" if s["fwd_splits"] > 1 else "") + (" packed-rows" if s["fwd_pack"] > 1 else "") + (" list" if s["fwd_list"] else "")


def bwd_label(s, d, extra=""):
    return "bwd d%d dq_nw=%d dkdv_nw=%d spill=%d%s%s" % (d, s["bwd_dq_nw"], s["bwd_dkdv_nw"], s["bwd_spill"], " list%d" % s["bwd_list"] if s["bwd_list"] else "", extra)


class Case:
    """Deviations of one probed case, kept on the device until done(): one host sync per case."""

    def __init__(self, what, dtype, record=True):
        self.what, self.dtype, self.dev, self.exact, self.explain, self.labels, self.record = what, dtype, {}, [], [], set(), record

    def add(self, label, decoder, value, explain=None):
        self.labels.add(label)
        self.dev.setdefault((label, decoder), []).append(value.reshape(()))
        if explain is not None:
            self.explain.append((decoder, explain))

    def zero(self, count, what):
        self.exact.append((count.reshape(()), what))

    def done(self):
        keys = list(self.dev)
        vals = torch.stack([torch.stack(self.dev[k]).max() for k in keys] + [c.double() for c, _ in self.exact]).cpu().tolist()
        bad = []
        for (label, dec), v in zip(keys, vals):
            if self.record:
                m = _MARGINS.setdefault((label, DN[self.dtype]), {"cases": 0})
                m[dec] = max(m.get(dec, 0.0), v)
            if not v < mp.THRESHOLD:
                bad.append("%s: %s deviates by %.4f (threshold %.2f)" % (label, dec, v, mp.THRESHOLD))
        for (_, what), v in zip(self.exact, vals[len(keys):]):
            if v != 0:
                bad.append("%s: %d elements" % (what, int(v)))
        for label in (self.labels if self.record else ()):
            _BOOK[label] = _BOOK.get(label, 0) + 1
            _MARGINS.setdefault((label, DN[self.dtype]), {"cases": 0})["cases"] += 1
        if bad:
            detail = []
            for dec, fn in self.explain:
                detail += [msg for msg, _, _ in fn()][:6]
            pytest.fail("mask probe, %s %s:\n  " % (self.what, DN[self.dtype]) + "\n  ".join(bad + detail[:24]))


def need(label_ok, at_least=20):
    """The pinned kernel must have been probed: at least 20 booked cases on labels that satisfy the predicate."""
    n = sum(c for l, c in _BOOK.items() if label_ok(l))
    assert n >= at_least, "only %d probed cases on the pinned kernel; booked: %s" % (n, {l: c for l, c in sorted(_BOOK.items())})


def pass_table(n_ps, hk, call):
    """(B, Hk) long: the pass the (b, kv head) slot carries in call `call`; calls_for(n_ps, hk) calls cover every pass of every entry."""
    return torch.tensor([[(call * hk + h + b) % n_p for h in range(hk)] for b, n_p in enumerate(n_ps)], dtype=torch.long)


def calls_for(n_ps, hk):
    return -(-max(n_ps) // hk)


@functools.lru_cache(maxsize=None)
def fwd_exp(sq, sk, mask, max_k, dv):
    return mp.fwd_expected(mp.visible(sq, sk, mask, max_k, DEV), mp.fwd_codes(sk, dv, DEV))


@functools.lru_cache(maxsize=None)
def rand_k(shape, dtype):
    g = torch.Generator().manual_seed(sum(shape))
    return torch.randn(shape, generator=g).to(device=DEV, dtype=dtype)


def heads_cfg(idx):
    """(B, Hk, ratio) in turn: Hk 1 or 2 with ratio 1, 2 and 4, H <= 4, B <= 2."""
    return [(1, 1, 1), (2, 1, 2), (1, 2, 2), (1, 1, 4), (2, 2, 1), (1, 1, 2)][idx % 6]


def what_of(sq, sk, mask, b, hk, ratio, d, extra=""):
    return "Sq %d Sk %d mask %s B %d H %d/%d d %d%s" % (sq, sk, mp.mask_name(mask), b, hk * ratio, hk, d, extra)


# ---------------------------------------------------------------- fixed-length forward ----------------------------------------------------------------
def probe_fwd(be, sq, sk, mask, dtype, d, dv, b, hk, ratio, softcap=0.0, given=None):
    """given: the mask handed to the kernel where it is NOT the one the decoders expect (the self-test at the end of this module)."""
    case = Case(what_of(sq, sk, mask, b, hk, ratio, d, " fwd" + (" softcap" if softcap else "")), dtype, record=given is None)
    km = given or mask
    vis = mp.visible(sq, sk, mask, None, DEV)
    codes, exp = mp.fwd_codes(sk, dv, DEV), fwd_exp(sq, sk, mask, None, dv)
    q = torch.zeros(b, sq, hk * ratio, d, device=DEV, dtype=dtype)
    k = rand_k((b, sk, hk, d), dtype)
    for call in range(calls_for([codes.shape[0]] * b, hk)):
        po = pass_table([codes.shape[0]] * b, hk, call)
        v = mp.fwd_values(codes, po, dtype)
        out, lse = be.fwd(q, k, v, None, None, 0.0, mp.SCALE, km[0], km[1], km[2], softcap, False, None)[:2]
        label = fwd_label(be.last_schedule(), d)
        for i in range(b):
            poh = po[i].repeat_interleave(ratio)
            r = mp.fwd_check(out[i], lse[i], vis, exp, poh)
            ex = functools.partial(mp.fwd_failures, out[i], lse[i], vis, exp, poh)
            for dec in ("count", "fine", "coarse"):
                case.add(label, dec, r[dec], ex if dec == "fine" else None)
            case.zero(r["exact"], "rows without a visible key: lse must be +inf and out exactly 0")
    case.done()


def cases(shapes, masks):
    """(index of the head configuration, (Sq, Sk), mask, dtype): the index is shape + mask, so a mask meets another configuration at every shape."""
    for (si, shape), (mi, mask), dtype in itertools.product(enumerate(shapes), enumerate(masks), DTYPES):
        yield si + mi, shape, mask, dtype


def fwd_sweep(be, d, dv=None, softcap=0.0, shapes=mp.SHAPES, masks=mp.MASKS):
    for idx, (sq, sk), mask, dtype in cases(shapes, masks):
        b, hk, ratio = heads_cfg(idx)
        probe_fwd(be, sq, sk, mask, dtype, d, dv or d, b, hk, ratio, softcap)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("nw", [4, 8, 16, 34, 38, 64])
def test_forward_schedules(be, knobs, nw, d):
    knobs.set("FA_FWD_NW", nw)
    fwd_sweep(be, d)
    kernel, waves = {4: ("fa_fwd_kernel", ",4,feat0,lockstep"), 8: ("fa_fwd_kernel", ",8,feat0,lockstep"), 16: ("fa_fwd_kernel", "pingpong"),
                     34: ("fa_fwd_il_kernel", ",%d,4," % d), 38: ("fa_fwd_il_kernel", ",%d,8," % d), 64: ("fa_fwd_w64_kernel<T,%d>" % d, "")}[nw]
    need(lambda l: l.startswith("fwd d%d " % d) and kernel in l and waves in l)


@pytest.mark.parametrize("d", [256, 96, 40])
def test_forward_lockstep_head_dims(be, knobs, d):
    """Head dim 256, 96 (trimmed) and 40 (run-time column bound) run the 4-wave lock-step kernel."""
    fwd_sweep(be, d)
    need(lambda l: l.startswith("fwd d%d " % d) and "fa_fwd_kernel<T,%d,4," % {256: 256, 96: 96, 40: 64}[d] in l)


def test_forward_v_head_dim_128_beside_192(be, knobs):
    fwd_sweep(be, 192, 128)
    need(lambda l: "fa_fwd_dv_kernel<T,192,128" in l)


@pytest.mark.parametrize("nw", [8, 64])
def test_forward_softcap(be, knobs, nw):
    """softcap(0) = 0: the same decode applies."""
    knobs.set("FA_FWD_NW", nw)
    fwd_sweep(be, 128, softcap=20.0)
    need(lambda l: ("fa_fwd_w64_kernel<T,128,softcap>" in l) if nw == 64 else ("fa_fwd_kernel<T,128,8," in l and "feat0" not in l))


@pytest.mark.parametrize("nw", [34, 38])
def test_forward_strict(be, knobs, nw):
    knobs.set("FA_STRICT", 1)
    knobs.set("FA_FWD_NW", nw)
    before = dict(_BOOK)
    fwd_sweep(be, 128)
    assert sum(c - before.get(l, 0) for l, c in _BOOK.items() if "fa_fwd_il_kernel<T,128,%d," % (nw - 30) in l) >= 20


# ---------------------------------------------------------------- packed batches ----------------------------------------------------------------
def packed_layout(lens_q, lens_k_alloc):
    cu_q = torch.tensor([0] + list(np.cumsum(lens_q)), dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([0] + list(np.cumsum(lens_k_alloc)), dtype=torch.int32, device=DEV)
    return cu_q, cu_k


PACKED_TILES = 6   # the packed batch six times over (36 entries): 72 dense 256-row blocks, enough for the work lists of every schedule (fa_api.cpp varlen_list_entries: >= 64)


def probe_varlen_fwd(be, mask, dtype, d, hk, ratio, seqused):
    lens_q, alloc = mp.PACKED_LENS_Q * PACKED_TILES, mp.PACKED_LENS_K * PACKED_TILES
    lens_k = mp.PACKED_SEQUSED_K * PACKED_TILES if seqused else alloc
    max_k = max(alloc)
    case = Case("packed batch %d x (lens_q %s lens_k %s) mask %s H %d/%d d %d%s" % (PACKED_TILES, mp.PACKED_LENS_Q, lens_k[:6], mp.mask_name(mask), hk * ratio, hk, d,
                                                                                    " seqused_k" if seqused else ""), dtype)
    cu_q, cu_k = packed_layout(lens_q, alloc)
    cq, ck = cu_q.tolist(), cu_k.tolist()
    q = torch.zeros(sum(lens_q), hk * ratio, d, device=DEV, dtype=dtype)
    k = rand_k((sum(alloc), hk, d), dtype)
    su = torch.tensor(lens_k, dtype=torch.int32, device=DEV) if seqused else None
    codes = [mp.fwd_codes(n, d, DEV) for n in lens_k]
    n_ps = [c.shape[0] for c in codes]
    for call in range(calls_for(n_ps, hk)):
        po = pass_table(n_ps, hk, call)
        v = torch.full((sum(alloc), hk, d), float("nan"), device=DEV, dtype=dtype) if seqused else torch.zeros(sum(alloc), hk, d, device=DEV, dtype=dtype)
        for i, n in enumerate(lens_k):   # (with seqused_k the rows behind an entry's used length hold NaN: a key read from there shows)
            v[ck[i]:ck[i] + n] = codes[i][po[i]].permute(1, 0, 2).to(dtype)
        out, lse = be.varlen_fwd(q, k, v, None, cu_q, cu_k, su, None, None, None, max(lens_q), max_k, 0.0, mp.SCALE, False, mask[0], mask[1], mask[2],
                                 0.0, False, None)[:2]
        label = fwd_label(be.last_schedule(), d) + " varlen"
        for i, (nq, n) in enumerate(zip(lens_q, lens_k)):
            if nq == 0:
                continue
            vis, exp = mp.visible(nq, n, mask, max_k, DEV), fwd_exp(nq, n, mask, max_k, d)
            o, l, poh = out[cq[i]:cq[i + 1]], lse[:, cq[i]:cq[i + 1]], po[i].repeat_interleave(ratio)
            r = mp.fwd_check(o, l, vis, exp, poh)
            ex = functools.partial(mp.fwd_failures, o, l, vis, exp, poh)
            for dec in ("count", "fine", "coarse"):
                case.add(label, dec, r[dec], ex if dec == "fine" else None)
            case.zero(r["exact"], "entry %d: rows without a visible key: lse must be +inf and out exactly 0" % i)
    case.done()


@pytest.mark.parametrize("work_list", [1, 0])
@pytest.mark.parametrize("nw", [34, 38, 64])
def test_packed_forward(be, knobs, nw, work_list):
    """The window of a packed batch is normalised by the batch's longest key sequence; once more with seqused_k shortening two entries of every tile.  The batch is
    the issue's six entries six times over, so that the schedule pre-pass runs (FA_VARLEN_LIST=1: the label must say ' list') or is switched off (=0: it must not)."""
    knobs.set("FA_FWD_NW", nw)
    knobs.set("FA_VARLEN_LIST", work_list)
    before = dict(_BOOK)
    for idx, (mask, dtype, seqused, d) in enumerate(itertools.product(mp.MASKS, DTYPES, (False, True), (64, 128))):
        _, hk, ratio = heads_cfg(idx)
        probe_varlen_fwd(be, mask, dtype, d, hk, ratio, seqused)
    kernel = {34: "fa_fwd_il_kernel", 38: "fa_fwd_il_kernel", 64: "fa_fwd_w64_kernel"}[nw]
    new = {l: c - before.get(l, 0) for l, c in _BOOK.items() if c > before.get(l, 0) and l.endswith(" varlen") and kernel in l}
    assert sum(c for l, c in new.items() if (" list" in l) == bool(work_list)) >= 20, new
    assert not any((" list" in l) != bool(work_list) for l in new), new


# ---------------------------------------------------------------- KV cache ----------------------------------------------------------------
def probe_kvcache(be, sq, mask, dtype, hk, ratio, splits, paged, append, mla=False, lens=mp.CACHE_LENS, cap=1024):
    d, dv = (576, 512) if mla else (128, 128)
    b = len(lens)
    lens = [min(n, cap - sq) for n in lens] if append else list(lens)
    tot = [n + (sq if append else 0) for n in lens]
    case = Case("KV cache Sq %d cache_seqlens %s%s mask %s H %d/%d d %d splits %d%s" % (sq, lens, " + append" if append else "", mp.mask_name(mask), hk * ratio, hk, d,
                                                                                     splits, " paged" if paged else ""), dtype)
    q = torch.zeros(b, sq, hk * ratio, d, device=DEV, dtype=dtype)
    codes = [mp.fwd_codes(n, dv, DEV) for n in tot]
    n_ps = [c.shape[0] for c in codes]
    per = cap // 256
    for call in range(calls_for(n_ps, hk)):
        po = pass_table(n_ps, hk, call)
        kl = rand_k((b, cap, hk, d), dtype).clone()                     # logical caches; what no length covers holds NaN
        vl = torch.full((b, cap, hk, dv), float("nan"), device=DEV, dtype=dtype)
        kn = vn = None
        if append:
            kn, vn = rand_k((b, sq, hk, d), dtype).clone(), torch.zeros(b, sq, hk, dv, device=DEV, dtype=dtype)
        for i in range(b):
            rows = codes[i][po[i]].permute(1, 0, 2).to(dtype)             # (tot, Hk, Dv)
            vl[i, :lens[i]] = rows[:lens[i]]
            kl[i, lens[i]:] = float("nan")
            if append:
                vn[i] = rows[lens[i]:]
        if mla:                                                           # V is the latent part of K: the codes go into k_cache[..., :512]
            kl[..., :dv] = vl
            if append:
                kn[..., :dv] = vn
                vn = kn[..., :dv]
        table = None
        if paged:
            order = torch.randperm(b * per + 2, device=DEV)
            table = order[: b * per].reshape(b, per).to(torch.int32)
            kc = torch.full((b * per + 2, 256, hk, d), float("nan"), device=DEV, dtype=dtype)
            kc[table.long().reshape(-1)] = kl.reshape(b * per, 256, hk, d)
            vc = kc[..., :dv] if mla else torch.full((b * per + 2, 256, hk, dv), float("nan"), device=DEV, dtype=dtype)
            if not mla:
                vc[table.long().reshape(-1)] = vl.reshape(b * per, 256, hk, dv)
        else:
            kc, vc = kl, (kl[..., :dv] if mla else vl)
        cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
        out, lse = be.fwd_kvcache(q, kc, vc, kn, vn, cl, None, None, None, None, table, None, None, mp.SCALE, mask[0], mask[1], mask[2], 0.0, True, splits)
        label = fwd_label(be.last_schedule(), d) + " kvcache" + (" paged" if paged else "") + (" append" if append else "")
        for i in range(b):
            vis, exp = mp.visible(sq, tot[i], mask, None, DEV), fwd_exp(sq, tot[i], mask, None, dv)
            poh = po[i].repeat_interleave(ratio)
            r = mp.fwd_check(out[i], lse[i], vis, exp, poh)
            ex = functools.partial(mp.fwd_failures, out[i], lse[i], vis, exp, poh)
            for dec in ("count", "fine", "coarse"):
                case.add(label, dec, r[dec], ex if dec == "fine" else None)
            case.zero(r["exact"], "entry %d (%d keys): rows without a visible key: lse must be +inf and out exactly 0" % (i, tot[i]))
    case.done()


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged256"])
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("pack", [1, 0])
def test_kvcache(be, knobs, pack, splits, paged):
    """Kernel id 1 behind fa_fwd_kvcache and its split-KV merge, head packing on and off at ratios 4 and 8; once with an append of Sq rows."""
    knobs.set("FA_PACK_GQA", pack)
    before = dict(_BOOK)
    for idx, (sq, mask, dtype) in enumerate(itertools.product(mp.CACHE_SQ, mp.CACHE_MASKS, DTYPES)):
        for ratio in ((4, 8) if sq <= 5 else ((4, 8)[(idx // 2) % 2],)):   # (the chunks short enough to be packed at both ratios: both)
            probe_kvcache(be, sq, mask, dtype, 1 if ratio == 8 else 2, ratio, splits, paged, append=False)
    probe_kvcache(be, 33, mp.CACHE_MASKS[0], torch.bfloat16, 2, 4, splits, paged, append=True)
    probe_kvcache(be, 5, mp.CACHE_MASKS[1], torch.float16, 1, 8, splits, paged, append=True)
    assert sum(c - before.get(l, 0) for l, c in _BOOK.items() if "fa_fwd_kernel<T,128" in l and " kvcache" in l) >= 20, _BOOK
    if splits != 1:
        need(lambda l: "+splitkv" in l and " kvcache" in l and "fa_fwd_kernel" in l)
    if pack:
        need(lambda l: "packed-rows" in l and " kvcache" in l and "fa_fwd_kernel" in l)


@pytest.mark.parametrize("splits", [1, 3, 0])
def test_mla_decode(be, knobs, splits):
    """Kernel id 7 (q / k 576, v / o 512 = k_cache[..., :512]): H / Hk (16, 1) and (8, 2), Sq 1, 5, 130, causal and (200, -1)."""
    masks = [mp.CACHE_MASKS[0], mp.CACHE_MASKS[2]]
    for (hk, ratio), sq, mask, dtype, paged in itertools.product(((1, 16), (2, 4)), (1, 5, 130), masks, DTYPES, (False, True)):
        probe_kvcache(be, sq, mask, dtype, hk, ratio, splits, paged, append=False, mla=True)
    probe_kvcache(be, 5, masks[0], torch.bfloat16, 2, 4, splits, False, append=True, mla=True)
    need(lambda l: "fa_fwd_mla_kernel" in l and (splits == 1 or "+splitkv" in l))


# ---------------------------------------------------------------- paged prefill ----------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_paged_prefill_on_the_w64_kernel(be, knobs, d):
    """NW 64 with a block table: packed queries against a shuffled page table, the rows behind a sequence's end hold NaN."""
    knobs.set("FA_FWD_NW", 64)
    page = 256
    for idx, ((sq, sk), mask, dtype) in enumerate(itertools.product([(320, 576), (513, 513)], mp.MASKS, DTYPES)):
        _, hk, ratio = heads_cfg(idx // 2)
        case = Case(what_of(sq, sk, mask, 1, hk, ratio, d, " paged prefill"), dtype)
        per = -(-sk // page)
        codes, exp, vis = mp.fwd_codes(sk, d, DEV), fwd_exp(sq, sk, mask, sk, d), mp.visible(sq, sk, mask, sk, DEV)
        cu_q, cu_k = packed_layout([sq], [sk])
        q = torch.zeros(sq, hk * ratio, d, device=DEV, dtype=dtype)
        for call in range(calls_for([codes.shape[0]], hk)):
            po = pass_table([codes.shape[0]], hk, call)
            table = torch.randperm(per + 2, device=DEV)[:per].reshape(1, per).to(torch.int32)
            kl = torch.full((per * page, hk, d), float("nan"), device=DEV, dtype=dtype)
            vl = kl.clone()
            kl[:sk] = rand_k((sk, hk, d), dtype)
            vl[:sk] = codes[po[0]].permute(1, 0, 2).to(dtype)
            kp = torch.full((per + 2, page, hk, d), float("nan"), device=DEV, dtype=dtype)
            vp = kp.clone()
            kp[table.long().reshape(-1)] = kl.reshape(per, page, hk, d)
            vp[table.long().reshape(-1)] = vl.reshape(per, page, hk, d)
            out, lse = be.varlen_fwd(q, kp, vp, None, cu_q, cu_k, None, None, table, None, sq, sk, 0.0, mp.SCALE, False, mask[0], mask[1], mask[2], 0.0, False, None)[:2]
            label = fwd_label(be.last_schedule(), d) + " varlen"
            poh = po[0].repeat_interleave(ratio)
            r = mp.fwd_check(out, lse, vis, exp, poh)
            for dec in ("count", "fine", "coarse"):
                case.add(label, dec, r[dec], functools.partial(mp.fwd_failures, out, lse, vis, exp, poh) if dec == "fine" else None)
            case.zero(r["exact"], "rows without a visible key: lse must be +inf and out exactly 0")
        case.done()
    need(lambda l: "fa_fwd_w64_kernel<T,%d,paged>" % d in l)


# ---------------------------------------------------------------- backward ----------------------------------------------------------------
def _bwd_call(be, varlen, dout, q, k, v, out, lse, mask, cu=None, maxes=None, seqused_k=None):
    if varlen:
        bufs = [torch.zeros_like(t) for t in (q, k, v)] if seqused_k is not None else [None] * 3   # (gradient rows past seqused_k are not written: they must stay 0)
        return be.varlen_bwd(dout, q, k, v, out, lse, bufs[0], bufs[1], bufs[2], cu[0], cu[1], None, maxes[0], maxes[1], 0.0, mp.SCALE, False, mask[0], mask[1], mask[2],
                             0.0, False, None, None, seqused_k=seqused_k)[:3]
    return be.bwd(dout, q, k, v, out, lse, None, None, None, None, 0.0, mp.SCALE, mask[0], mask[1], mask[2], 0.0, False, None, None)[:3]


def plan_of(b, sq, sk, h, hk, d, mask, dtype):
    """fa_bwd_plan_query of a fixed-length call: out[0] = launch kind (0 = the dQ + dK/dV pair), out[3] = virtual kv heads a GQA group is split into (0 = unsplit)."""
    import ctypes as C
    from flash_attn_amd import _cabi
    a = _cabi.FaBwdParams()
    a.b, a.h, a.h_k, a.d = b, h, hk, d
    a.seqlen_q, a.seqlen_k, a.total_q, a.total_k = sq, sk, b * sq, b * sk
    a.dtype = _cabi.FA_DTYPE_BF16 if dtype == torch.bfloat16 else _cabi.FA_DTYPE_FP16
    a.softmax_scale, a.is_causal, a.window_left, a.window_right = mp.SCALE, int(mask[0]), mask[1], mask[2]
    out = (C.c_int32 * 8)()
    assert _cabi.load().fa_bwd_plan_query(C.byref(a), out, 8) == 8
    return list(out)


def probe_bwd(be, seqs, mask, dtype, d, dv, hk, ratio, varlen=False, extra="", max_k=None, given=None, alloc=None, only=None, plan=False):
    """seqs: [(Sq, Sk)] -- the entries of a fixed-length batch (all equal) or of a packed one; alloc: the key rows each packed entry owns where seqused_k makes it
    use fewer (the rows behind hold finite fillers: a key read from there shows as a wrong count).  The dV probe (v = 0: dQ and dK exactly 0), then the dQ probe
    with both sign codes (dK exactly 0); dV of every key row that no probed query can see -- entries without queries, rows behind seqused_k -- exactly 0.
    only: "dv" / "dq" = that probe alone.  plan: the label says what fa_bwd_plan_query reports for the group split."""
    b, h = len(seqs), hk * ratio
    used = [s[1] for s in seqs]
    alloc = used if alloc is None else alloc
    shortened = alloc != used
    case = Case(("packed batch %d entries %s.." % (b, seqs[:6]) if varlen else "Sq %d Sk %d B %d" % (seqs[0] + (b,))) +
                " mask %s H %d/%d d %d/%d bwd%s%s" % (mp.mask_name(mask), h, hk, d, dv, extra, " seqused_k" if shortened else ""), dtype, record=given is None)
    km = given or mask
    if plan:
        pl = plan_of(b, seqs[0][0], seqs[0][1], h, hk, d, mask, dtype)
        extra += " plan=%d gsplit=%d" % (pl[0], pl[3])
    cu = packed_layout([s[0] for s in seqs], alloc) if varlen else None
    su = torch.tensor(used, dtype=torch.int32, device=DEV) if shortened else None
    maxes = (max(s[0] for s in seqs), max(alloc))
    cq, ck = (cu[0].tolist(), cu[1].tolist()) if varlen else (None, None)
    live = [i for i, (nq, nk) in enumerate(seqs) if nq > 0]

    def pack(ts):   # per-entry tensors (rows, heads, width) -> the call's layout
        return torch.cat(ts, 0) if varlen else torch.stack(ts, 0)

    def keys(ts, fill):   # the same for key rows: an entry's used rows, then a filler up to the rows it owns
        return pack([torch.cat([t, torch.full((n - t.shape[0],) + t.shape[1:], fill, device=DEV, dtype=dtype)], 0) if n > t.shape[0] else t for t, n in zip(ts, alloc)])

    def entry(t, i, key_rows):
        if not varlen:
            return t[i]
        return t[ck[i]:ck[i] + used[i]] if key_rows else t[cq[i]:cq[i + 1]]

    def unseen(t):   # key rows of a packed batch that no probed query sees
        if not varlen:
            return t[:0]
        seen = torch.zeros(t.shape[0], dtype=torch.bool, device=DEV)
        for i in live:
            seen[ck[i]:ck[i] + used[i]] = True
        return t[~seen]

    viss = [mp.visible(nq, nk, mask, max_k, DEV) for nq, nk in seqs]
    lse_e = [mp.ref_lse(vv)[None].expand(h, -1) for vv in viss]
    lse = torch.cat(lse_e, 1).contiguous() if varlen else torch.stack(lse_e, 0).contiguous()
    q = pack([torch.zeros(nq, h, d, device=DEV, dtype=dtype) for nq, _ in seqs])
    krand = keys([rand_k((nk, hk, d), dtype) for _, nk in seqs], 1.0)
    zero_o = pack([torch.zeros(nq, h, dv, device=DEV, dtype=dtype) for nq, _ in seqs])
    if only != "dq":
        pr = [mp.dv_probe(nq, nk, mask, dv, ratio, max_k, DEV) for nq, nk in seqs]
        n_ps = [p[0].shape[0] for p in pr]
        zv = keys([torch.zeros(nk, hk, dv, device=DEV, dtype=dtype) for _, nk in seqs], 3.0)
        for call in range(calls_for(n_ps, hk)):
            po = pass_table(n_ps, hk, call)
            dout = pack([mp.dv_dout(pr[i][0], po[i:i + 1], dtype)[0] for i in range(b)])
            dq, dk, dvv = _bwd_call(be, varlen, dout, q, krand, zv, zero_o, lse, km, cu, maxes, su)
            label = bwd_label(be.last_schedule(), d, extra)
            for i in live:
                g = entry(dvv, i, True)
                case.add(label, "dv", mp.dv_check(g, pr[i][1], po[i]), functools.partial(mp.dv_failures, g, pr[i][1], po[i], seqs[i][0], ratio))
            case.zero(mp.exact_zero(dq), "dQ of the dV probe (v = 0) must be exactly 0")
            case.zero(mp.exact_zero(dk), "dK of the dV probe (q = 0) must be exactly 0")
            case.zero(mp.exact_zero(unseen(dvv)), "dV of key rows that no query sees (an entry without queries, rows behind seqused_k) must be exactly 0")
    for code in ((0, 1) if only != "dv" else ()):
        pq = [mp.dq_probe(nq, nk, mask, d, code, dtype, max_k, DEV) for nq, nk in seqs]
        n_ps = [p[2].shape[0] for p in pq]
        vs, dos, outs = [], [], []
        for (nq, nk), (a, o0, _, _) in zip(seqs, pq):
            vv = torch.zeros(nk, hk, dv, device=DEV, dtype=dtype); vv[:, :, 0] = a.to(dtype)[:, None]
            dd = torch.zeros(nq, h, dv, device=DEV, dtype=dtype); dd[:, :, 0] = 1
            oo = torch.zeros(nq, h, dv, device=DEV, dtype=dtype); oo[:, :, 0] = o0[:, None]
            vs.append(vv); dos.append(dd); outs.append(oo)
        v, dout, out = keys(vs, 3.0), pack(dos), pack(outs)
        for call in range(calls_for(n_ps, hk)):
            po = pass_table(n_ps, hk, call)
            k = keys([mp.dq_keys(pq[i][2], po[i:i + 1], dtype)[0] for i in range(b)], 1.0)
            dq, dk, _ = _bwd_call(be, varlen, dout, q, k, v, out, lse, km, cu, maxes, su)
            label = bwd_label(be.last_schedule(), d, extra)
            for i in live:
                g, poh = entry(dq, i, False), po[i].repeat_interleave(ratio)
                dev, ex = mp.dq_check(g, viss[i], pq[i][3], poh)
                case.add(label, "dq", dev, functools.partial(mp.dq_failures, g, viss[i], pq[i][3], poh))
                case.zero(ex, "dQ of rows without a visible key must be exactly 0")
            case.zero(mp.exact_zero(dk), "dK of the dQ probe (q = 0) must be exactly 0")
    case.done()


def bwd_sweep(be, d, dv=None, shapes=mp.SHAPES, masks=mp.MASKS, cfg=heads_cfg, extra="", plan=False):
    for idx, (sq, sk), mask, dtype in cases(shapes, masks):
        b, hk, ratio = cfg(idx)
        probe_bwd(be, [(sq, sk)] * b, mask, dtype, d, dv or d, hk, ratio, extra=extra, plan=plan)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dkdv", [8, 64])
@pytest.mark.parametrize("dq_nw", [4, 8, 64])
def test_backward_recomputing_pair(be, knobs, dq_nw, dkdv, d):
    knobs.set("FA_BWD_GSPLIT", 0)
    knobs.set("FA_BWD_MODE", -1)
    knobs.set("FA_BWD_DQ_NW", dq_nw)
    knobs.set("FA_BWD_DKDV", dkdv)
    bwd_sweep(be, d)
    need(lambda l: l.startswith("bwd d%d dq_nw=%d dkdv_nw=%d spill=0" % (d, dq_nw, dkdv)))


@pytest.mark.parametrize("d", [256, 96, 40])
def test_backward_four_wave_head_dims(be, knobs, d):
    knobs.set("FA_BWD_GSPLIT", 0)
    knobs.set("FA_BWD_MODE", -1)
    bwd_sweep(be, d)
    need(lambda l: l.startswith("bwd d%d dq_nw=4 " % d))


def test_backward_v_head_dim_128_beside_192(be, knobs):
    knobs.set("FA_BWD_GSPLIT", 0)
    bwd_sweep(be, 192, 128)
    need(lambda l: l.startswith("bwd d192 dq_nw=4 "))


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("mode", [3, 5])
def test_backward_fused_and_chunked_launches(be, knobs, mode, d):
    """FA_BWD_MODE=3 (one fused launch) and =5 (chunked mixed launches) on the shapes they accept: Sk >= Sq, no left window."""
    knobs.set("FA_BWD_GSPLIT", 0)
    knobs.set("FA_BWD_MODE", mode)
    shapes = [s for s in mp.SHAPES if s[1] >= s[0]]
    masks = [m for m in mp.MASKS if m[1] < 0]
    bwd_sweep(be, d, shapes=shapes, masks=masks)
    need(lambda l: l.startswith("bwd d%d " % d) and "spill=%d" % mode in l)


@pytest.mark.parametrize("gsplit", [0, 16])
def test_backward_group_split(be, knobs, monkeypatch, gsplit):
    """FA_BWD_GSPLIT 0 and 16 at ratios 4 and 8 (16 forces the split of a group into virtual kv heads: fa_api.cpp bwd_gsplit_plan).  last_schedule() does not say
    whether the split ran, so the case is booked under what fa_bwd_plan_query reports for the call, and -- the launch falls back to the unsplit kernels where no
    workspace arrives (launch_dkdv_any) -- the binder must have allocated a workspace for every split call and none for an unsplit one; last, as
    tests/test_bwd_gsplit_gpu.py does, dK of a split run on random inputs differs from the unsplit run's (the partials are rounded to the dtype before the sum)."""
    knobs.set("FA_BWD_GSPLIT", gsplit)
    knobs.set("FA_BWD_MODE", -1)
    allocs, real = [], be._alloc_workspace
    monkeypatch.setattr(be, "_alloc_workspace", lambda n, dev: (allocs.append(n), real(n, dev))[1])
    calls, real_bwd = [], be.bwd
    monkeypatch.setattr(be, "bwd", lambda *a: (calls.append(1), real_bwd(*a))[1])
    shapes = [(65, 65), (129, 257), (257, 129), (513, 513), (300, 1100)]
    bwd_sweep(be, 128, shapes=shapes, cfg=lambda idx: [(1, 1, 4), (1, 1, 8), (2, 1, 4)][idx % 3], plan=True)
    if gsplit:
        assert len(allocs) == len(calls) and min(allocs) > 0, (len(allocs), len(calls))
        need(lambda l: l.startswith("bwd d128 ") and (l.endswith(" plan=0 gsplit=4") or l.endswith(" plan=0 gsplit=8")))
        assert sum(c for l, c in _BOOK.items() if l.endswith(" plan=0 gsplit=8")) >= 20 and sum(c for l, c in _BOOK.items() if l.endswith(" plan=0 gsplit=4")) >= 20, _BOOK
        torch.manual_seed(3)
        q = torch.randn(1, 513, 8, 128, device=DEV, dtype=torch.bfloat16)
        k, v, do = torch.randn(1, 513, 1, 128, device=DEV, dtype=torch.bfloat16), torch.randn(1, 513, 1, 128, device=DEV, dtype=torch.bfloat16), torch.randn_like(q)
        grads = {}
        for gs in (16, 0):
            knobs.set("FA_BWD_GSPLIT", gs)
            out, lse = be.fwd(q, k, v, None, None, 0.0, mp.SCALE, True, -1, -1, 0.0, False, None)[:2]
            grads[gs] = real_bwd(do, q, k, v, out, lse, None, None, None, None, 0.0, mp.SCALE, True, -1, -1, 0.0, False, None, None)
        assert torch.equal(grads[16][0], grads[0][0]) and not torch.equal(grads[16][1], grads[0][1]) and not torch.equal(grads[16][2], grads[0][2]), "the forced split ran"
    else:
        assert not allocs, allocs   # (the recomputing pair of an unsplit fixed-length call needs no workspace)
        need(lambda l: l.startswith("bwd d128 ") and l.endswith(" plan=0 gsplit=0"))


@pytest.mark.parametrize("work_list", [1, 0])
@pytest.mark.parametrize("d", [64, 128])
def test_packed_backward(be, knobs, d, work_list):
    """The packed batch through varlen_bwd, plain and with seqused_k, six times over so that the query-block and key-block work lists run (bwd_list = 3) or are
    switched off (FA_VARLEN_LIST=0)."""
    knobs.set("FA_BWD_GSPLIT", 0)
    knobs.set("FA_VARLEN_LIST", work_list)
    before = dict(_BOOK)
    lens_q, alloc = mp.PACKED_LENS_Q * PACKED_TILES, mp.PACKED_LENS_K * PACKED_TILES
    for idx, (mask, dtype, seqused) in enumerate(itertools.product(mp.MASKS, DTYPES, (False, True))):
        _, hk, ratio = heads_cfg(idx)
        used = mp.PACKED_SEQUSED_K * PACKED_TILES if seqused else alloc
        probe_bwd(be, list(zip(lens_q, used)), mask, dtype, d, d, hk, ratio, varlen=True, extra=" varlen", max_k=max(alloc), alloc=alloc)
    new = {l: c - before.get(l, 0) for l, c in _BOOK.items() if c > before.get(l, 0) and l.startswith("bwd d%d " % d) and l.endswith(" varlen")}
    assert sum(c for l, c in new.items() if (" list3" in l) == bool(work_list)) >= 20, new
    assert not any((" list" in l) != bool(work_list) for l in new), new


# ---------------------------------------------------------------- default dispatch ----------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_default_dispatch(be, knobs, d):
    """No knobs: whatever the tables pick on (513, 513), (1024, 1024) and (300, 1100) under every mask must pass the probe, forward and backward."""
    for name in ("FA_FWD_NW", "FA_BWD_DQ_NW", "FA_BWD_DKDV", "FA_BWD_MODE", "FA_BWD_GSPLIT", "FA_STRICT", "FA_PACK_GQA", "FA_VARLEN_LIST"):
        knobs.unset(name)
    shapes = [(513, 513), (1024, 1024), (300, 1100)]
    fwd_sweep(be, d, shapes=shapes)
    bwd_sweep(be, d, shapes=shapes, extra=" default", plan=True)
    need(lambda l: l.startswith("bwd d%d " % d) and " default" in l)


# ---------------------------------------------------------------- the probe can fail here too ----------------------------------------------------------------
@pytest.mark.parametrize("given", [(False, 63, 1), (False, 64, 0), (False, 62, 0), (True, -1, -1)], ids=["wr+1", "wl+1", "wl-1", "no_left_bound"])
def test_a_kernel_given_another_window_is_reported(be, knobs, given):
    """The kernels are handed a window that is one key off the one the decoders expect (tests/test_mask_probe_cpu.py does this to a stand-in with every wrong mask of
    its list): the forward, the dV probe and the dQ probe must each report it, with the row or key in the message.  Nothing of this is booked or written to the margins file."""
    knobs.set("FA_BWD_GSPLIT", 0)
    for dtype, (sq, sk) in itertools.product(DTYPES, [(129, 257), (513, 513)]):
        with pytest.raises(pytest.fail.Exception, match=r"identity: head \d+ row \d+"):
            probe_fwd(be, sq, sk, (False, 63, 0), dtype, 128, 128, 1, 1, 2, given=given)
        with pytest.raises(pytest.fail.Exception, match=r"dV: kv head \d+ key \d+"):
            probe_bwd(be, [(sq, sk)], (False, 63, 0), dtype, 128, 128, 1, 2, given=given, only="dv")
        with pytest.raises(pytest.fail.Exception, match=r"dQ: head \d+ row \d+"):
            probe_bwd(be, [(sq, sk)], (False, 63, 0), dtype, 128, 128, 1, 2, given=given, only="dq")
