"""Does every dropout kernel keep EXACTLY the pairs the documented stream keeps?  The parity tests of dropout take their mask from the lock-step forward's
return_softmax payload and judge out / dq / dk / dv by an error bound; a few wrong pairs (the wrong byte of a word at Sk % 4 != 0, a tile-local key group, the
kv head for the query head, < for <=) stay below it, and the 64-rows-per-wave forward writes no payload at all.  Here the expected keep set comes from a host
model of DESIGN.md section 3.3 (tests/_dropout_model.py) and is decoded exactly with q = 0 (tests/_dropout_probe.py: the construction, the cap, the derived
0.25 threshold); tests/test_dropout_probe_cpu.py shows that the probe reports each of thirteen wrong keep sets and proves the kernel list below complete.

  a. payload == model: the bytes fa_fwd / fa_varlen_fwd return equal rand_bytes(rng_state) bit for bit.  Read from csrc/fa_fwd.hip: a processed 64-key tile
     writes the byte of EVERY key < Sk of a valid row, masked or not ("if (rv_row && row_valid && key0 + c < sk) rv_row[key0 + c] = (uint8_t)byte;"), a
     skipped tile writes nothing and the binder zero-fills the payload.  So: equal on every visible pair; on an invisible pair equal or still 0.
     This is the ONLY comparison that touches the payload; no test here reads a keep mask from the code it then judges.
  b. the forward probe on every mask-drawing forward key of the census, c. the dV and dQ probes on every mask-drawing backward key (rng_state is a tensor the
     test writes, so seeds >= 2^40 and offsets >= 2^32 are exercised directly), d. the GQA group split, e. the public functions under autograd.

Every pinned case takes its knobs from the census recipe that claims the kernel (tests/_kernel_census.py), plus FA_BWD_MODE=1 / FA_BWD_GSPLIT=0 where the
recipe has them, runs with FA_DEBUG_LAUNCH_LOG=1 and asserts that every mask-drawing key of the recipe is in the launch log of the probed calls under no mask
AND under the causal mask.  Shapes: B = 2, H = 4, Hk = 2 (b, query head and kv head all differ): (65, 130) Sk % 4 = 2 and one partial tile; (129, 257) the
128-row and 256-key seams, Sk % 4 = 1; (293, 331) the census backward shape, a second 256-row block, Sk % 4 = 3; (300, 1100) five key blocks, for the
64-rows-per-wave kernels and the default dispatch only.  bf16 runs shapes x masks; fp16 does the same at D = 128 and the census shape under none / causal elsewhere.
With FA_DROPOUT_PROBE_MARGINS=<file> the worst deviation per decoder, kernel family and dtype is written there (profiles/dropout_probe_margins.txt)."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import _dropout_model as dm
from tests import _dropout_probe as dp
from tests import _kernel_census as kc
from tests import _mask_probe as mp

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, HK = 2, 4, 2
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
SHAPES = [(65, 130), (129, 257), (293, 331)]
BIG = (300, 1100)
MASKS = [(False, -1, -1), (True, -1, -1), (False, 100, 50), (False, 64, 0)]
# (seed, offset): high words set / clear in turn; offsets are multiples of 4 as the generator requires
RNGS = [(0x123456789ABC, (1 << 32) + 64), (42, 8), ((1 << 40) + 5, 16), (77, (5 << 32) + 128)]
OTHER_P = [0.17, 0.6, 0.999, 0.001]
PACKED_TILES = 6   # the packed batch six times over, so that the work lists of every schedule run (as tests/test_mask_probe_gpu.py)
MASK_FAMILIES = ("fa_fwd_kernel", "fa_fwd_w64_kernel", "fa_bwd_dq_kernel", "fa_bwd_dkdv_kernel", "fa_bwd_dq_w64_kernel")
_FEAT_AT = {"fa_fwd_kernel": 3, "fa_fwd_w64_kernel": 1, "fa_bwd_dq_kernel": 3, "fa_bwd_dkdv_kernel": 2, "fa_bwd_dq_w64_kernel": 2}
_MARGINS = {}   # {(family label, dtype name): {decoder: worst, "cases": n}}


def draws_mask(key):
    """A census key whose code object can draw a dropout mask: its feature code has the DROP bit (FEAT_ALL = 7 has it)."""
    family, _, args = key
    return family in MASK_FAMILIES and bool(args[_FEAT_AT[family]] & kc.DROP) and args[_FEAT_AT[family]] != kc.EXACT


def _pinned():
    """One entry per distinct (knobs, mask-drawing keys) of the census' attention recipes: id, dt, d, the call's features and the keys by side."""
    seen, rows = set(), []
    for r in kc.RECIPES:
        keys = tuple(k for k in r["keys"] if draws_mask(k))
        if r["kind"] != "attn" or not keys:
            continue
        ident = (tuple(sorted(r["knobs"].items())), keys)
        if ident in seen:
            continue
        seen.add(ident)
        rid = r["id"]
        for mode in ("-full", "-causal", "-local"):
            rid = rid[:-len(mode)] if rid.endswith(mode) else rid
        rows.append(dict(id=rid, dt=r["dt"], d=r["d"], cap=20.0 if r["cap"] else 0.0, alibi=bool(r["alibi"]), knobs=dict(r["knobs"]),
                         fwd_keys=[k for k in keys if k[0].startswith("fa_fwd")], bwd_keys=[k for k in keys if k[0].startswith("fa_bwd")]))
    return rows


PINNED = _pinned()


def schedule(row):
    """[(shape, mask, p, rng)] of a pinned entry: bf16 (and fp16 at D = 128) shapes x masks, fp16 elsewhere the census shape under none / causal; p = 0.5."""
    w64 = any("w64" in k[0] for k in row["fwd_keys"] + row["bwd_keys"])
    wide = row["dt"] == "bf16" or row["d"] == 128
    shapes = (SHAPES + ([BIG] if w64 else [])) if wide else [SHAPES[2]]
    masks = MASKS if wide else MASKS[:2]
    return [(s, m, 0.5, RNGS[(si + mi) % len(RNGS)]) for (si, s), (mi, m) in itertools.product(enumerate(shapes), enumerate(masks))]


def numeric_cases():
    """Every distinct (packed, seqs / shape, mask, p, rng, d, dtype name) this module probes at H / Hk = 4 / 2: what tests/test_dropout_probe_cpu.py runs the
    stand-in over.  Left out, as restatements of these on other head counts or lengths: the H / Hk = 8 / 1 half of the group-split test and the padded batch of
    the public-function test (the same shape class with two entries shortened)."""
    out = set()
    for row in PINNED:
        for s, m, p, rng in schedule(row):
            out.add((False, s, m, p, rng, row["d"], row["dt"]))
    for p, m, dt in itertools.product(OTHER_P, MASKS[:2], ("bf16",)):
        out.add((False, SHAPES[2], m, p, RNGS[0], 128, dt))
    for m, d in itertools.product(MASKS, (64, 128)):
        out.add((True, None, m, 0.5, RNGS[0], d, "bf16"))
    for m in MASKS[:2]:
        out.add((False, BIG, m, 0.5, RNGS[3], 128, "bf16"))
    return sorted(out, key=repr)


def packed_seqs(tiles=1):
    return list(zip(mp.PACKED_LENS_Q * tiles, mp.PACKED_LENS_K * tiles))


# ---------------------------------------------------------------- plumbing ----------------------------------------------------------------
@pytest.fixture(scope="module")
def be():
    from flash_attn_amd import backend
    return backend


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    yield
    dp.clear_caches()
    mp.clear_caches()
    torch.cuda.empty_cache()
    path = os.environ.get("FA_DROPOUT_PROBE_MARGINS")
    if path and _MARGINS:
        decs = ("count", "fine", "coarse", "dv", "dq")
        with open(path, "w") as f:
            f.write("# worst deviation of each decoder of the dropout probe (tests/test_dropout_probe_gpu.py) per kernel family and dtype; threshold 0.25 (dV of a split group 0.375)\n"
                    "# family                                             dtype  cases   " + "".join("%9s" % d for d in decs) + "\n")
            for (label, dn), m in sorted(_MARGINS.items()):
                f.write("%-52s %-5s %6d   " % (label, dn, m["cases"]) + "".join(("%9.4f" % m[d]) if d in m else "%9s" % "-" for d in decs) + "\n")


class Run:
    """One pinned kernel under probe: the knobs, the launch log of every probed call booked per mask, the calls handed to the probe helpers."""

    def __init__(self, be, knobs, knob_values, label):
        self.be, self.label, self.ran, self.knobs, self.names = be, label, {}, knobs, list(knob_values) + ["FA_W64_PERSIST"]
        for name, value in dict(knob_values, FA_DEBUG_LAUNCH_LOG=1).items():
            knobs.set(name, value)

    def close(self):
        """Take this run's schedule knobs back, so that the next pinned kernel of the same test starts from the defaults."""
        for name in self.names:
            self.knobs.unset(name)

    def book(self, mask):
        log = self.be.launch_log()
        assert "?" not in log and "?overflow" not in log, log
        for s in log:
            self.ran.setdefault(kc.parse_symbol(s), set()).add(mp.mask_name(mask))

    def assert_ran(self, keys, masks=("none", "causal")):
        for k in keys:
            got = self.ran.get(k, set())
            assert set(masks) <= got, "%s ran under %s only; launched: %s" % (kc.key_str(k), sorted(got), sorted(kc.key_str(x) for x in self.ran if x))

    def finish(self, res, what, dtype, dv_threshold=dp.THRESHOLD):
        worst, exact = res.worst()
        m = _MARGINS.setdefault((self.label, "bf16" if dtype == torch.bfloat16 else "fp16"), {"cases": 0})
        m["cases"] += 1
        bad = []
        for dec, v in worst.items():
            m[dec] = max(m.get(dec, 0.0), v)
            thr = dv_threshold if dec == "dv" else dp.THRESHOLD
            print("dropout probe %s | %s | %s deviation %.4f (threshold %.3f)" % (self.label, what, dec, v, thr))
            if not v < thr:
                bad.append("%s deviates by %.4f (threshold %.3f)" % (dec, v, thr))
        if exact:
            bad += ["%s: %d elements" % (w, int(c)) for c, w in res.zeros if int(c)]
        if bad:
            detail = []
            for _, v, ex in res.devs:
                if ex is not None and not float(v) < dp.THRESHOLD and len(detail) < 18:
                    detail += [f[0] for f in ex()][:6]
            pytest.fail("dropout probe, %s, %s:\n  " % (self.label, what) + "\n  ".join(bad + detail[:18]))


def set_generator(seed, offset):
    torch.manual_seed(seed)
    torch.cuda.default_generators[torch.cuda.current_device()].set_offset(offset)


def rng_tensor(rng):
    return torch.tensor([x - (1 << 64) if x >= (1 << 63) else x for x in rng], dtype=torch.int64, device=DEV)


def _alibi(on, nb, h=H):
    return torch.zeros(nb, h, dtype=torch.float32, device=DEV) if on else None


def calls(run, pb, cap=0.0, alibi=False, packed=False, return_softmax=False, seqused=None):
    """(fwd, bwd) for dp.probe_*: fixed-length (stack) or packed (cat) calls of the ctypes binder under the Problem's mask, p and rng."""
    be, m, nb = run.be, pb.mask, len(pb.seqs)
    al = _alibi(alibi, nb, pb.h)
    rt = rng_tensor(pb.rng)
    if packed:
        cu_q = torch.tensor([0] + list(np.cumsum([s[0] for s in pb.seqs])), dtype=torch.int32, device=DEV)
        cu_k = torch.tensor([0] + list(np.cumsum([s[1] for s in pb.seqs])), dtype=torch.int32, device=DEV)
        cq, ck = cu_q.tolist(), cu_k.tolist()
        mq, mk = max(s[0] for s in pb.seqs), max(s[1] for s in pb.seqs)

    def fwd(q_e, k_e, v_e):
        set_generator(*pb.rng)
        if packed:
            out, lse, _, rng = be.varlen_fwd(torch.cat(q_e), torch.cat(k_e), torch.cat(v_e), None, cu_q, cu_k, None, None, None, al, mq, mk, pb.p, dp.SCALE, False,
                                             m[0], m[1], m[2], cap, return_softmax, None)
            res = [(out[cq[b]:cq[b + 1]], lse[:, cq[b]:cq[b + 1]]) for b in range(nb)]
        else:
            out, lse, _, rng = be.fwd(torch.stack(q_e), torch.stack(k_e), torch.stack(v_e), None, al, pb.p, dp.SCALE, m[0], m[1], m[2], cap, return_softmax, None)
            res = [(out[b], lse[b]) for b in range(nb)]
        run.book(m)
        assert torch.equal(rng, rt), "rng_state is the generator's (seed, offset)"
        return res

    def bwd(do_e, q_e, k_e, v_e, o_e, l_e):
        if packed:
            dq, dk, dv = be.varlen_bwd(torch.cat(do_e), torch.cat(q_e), torch.cat(k_e), torch.cat(v_e), torch.cat(o_e), torch.cat(l_e, 1).contiguous(), None, None, None,
                                       cu_q, cu_k, al, mq, mk, pb.p, dp.SCALE, False, m[0], m[1], m[2], cap, False, None, rt)[:3]
            res = [(dq[cq[b]:cq[b + 1]], dk[ck[b]:ck[b + 1]], dv[ck[b]:ck[b + 1]]) for b in range(nb)]
        else:
            dq, dk, dv = be.bwd(torch.stack(do_e), torch.stack(q_e), torch.stack(k_e), torch.stack(v_e), torch.stack(o_e), torch.stack(l_e), None, None, None,
                                al, pb.p, dp.SCALE, m[0], m[1], m[2], cap, False, None, rt)[:3]
            res = [(dq[b], dk[b], dv[b]) for b in range(nb)]
        run.book(m)
        return res
    return fwd, bwd


def scores_check(cap, alibi):
    return lambda q, k: dp.assert_uniform_scores(q, k, cap, torch.zeros(q.shape[1], device=DEV) if alibi else None)


def problem(shape, mask, p, rng, d, dtype, packed_tiles=0):
    if packed_tiles:
        seqs = packed_seqs(packed_tiles)
        return dp.Problem(seqs, mask, p, rng, H, HK, d, d, dtype, DEV, max_k=max(s[1] for s in seqs))
    return dp.Problem([shape] * B, mask, p, rng, H, HK, d, d, dtype, DEV)


def what_of(pb, extra=""):
    return "%s mask %s p %g rng (%#x, %#x) d %d%s" % (pb.seqs[0] if len(pb.seqs) == B else "packed x%d" % (len(pb.seqs) // 6), mp.mask_name(pb.mask), pb.p, pb.rng[0], pb.rng[1], pb.d, extra)


def probe_forward(run, pb, cap=0.0, alibi=False, packed=False, return_softmax=False, extra=""):
    fwd, _ = calls(run, pb, cap, alibi, packed, return_softmax)
    run.finish(dp.probe_fwd(pb, fwd, scores_check(cap, alibi)), what_of(pb, " fwd" + extra), pb.dtype)


def probe_backward(run, pb, cap=0.0, alibi=False, packed=False, extra="", dv_threshold=dp.THRESHOLD):
    _, bwd = calls(run, pb, cap, alibi, packed)
    run.finish(dp.probe_dv(pb, bwd, scores_check(cap, alibi)), what_of(pb, " dV" + extra), pb.dtype, dv_threshold)
    run.finish(dp.probe_dq(pb, bwd, scores_check(cap, alibi)), what_of(pb, " dQ" + extra), pb.dtype)


def family_label(row):
    fams = sorted({k[0] for k in row["fwd_keys"] + row["bwd_keys"]})
    return "%s d%d %s" % ("+".join(f.replace("fa_", "").replace("_kernel", "") for f in fams), row["d"], row["id"].split("-", 2)[-1] if row["id"].count("-") >= 2 else row["id"])


# ---------------------------------------------------------------- a. payload == model ----------------------------------------------------------------
def _check_payload(rv, vis, model, what):
    """rv, model uint8 (H, Sq, Sk); vis (Sq, Sk)."""
    v = vis[None].expand_as(rv)
    wrong = int((v & (rv != model)).sum())
    stray = int((~v & (rv != model) & (rv != 0)).sum())
    if wrong or stray:
        at = torch.nonzero(v & (rv != model))[:4].tolist() + torch.nonzero(~v & (rv != model) & (rv != 0))[:4].tolist()
        pytest.fail("%s: %d visible pairs whose byte differs from the model, %d invisible pairs neither the model's byte nor 0; first (head, row, key): %s"
                    % (what, wrong, stray, [(h, i, j, int(rv[h, i, j]), int(model[h, i, j])) for h, i, j in at]))


FEATURES = [("drop", 0.0, False), ("cap+drop", 20.0, False), ("alibi+drop", 0.0, True), ("all", 20.0, True)]


@pytest.mark.parametrize("d,nw", [(64, 4), (64, 8), (128, 4), (128, 8), (256, 4), (96, 4)])
def test_payload_equals_model(be, knobs, d, nw):
    """fa_fwd with return_softmax on the lock-step kernel, D = 64 / 128 / 256 and the trimmed 96, 4 and 8 waves, the four feature variants; random q / k / v
    (the bytes do not depend on the data); seeds >= 2^40 through torch.manual_seed and offsets >= 2^32 through the default generator's set_offset."""
    if d in (64, 128):
        knobs.set("FA_FWD_NW", nw)
    g = torch.Generator().manual_seed(d + nw)
    for (fi_, (feature, cap, alibi)), (si, (sq, sk)), (mi, mask) in itertools.product(enumerate(FEATURES), enumerate(SHAPES), enumerate(MASKS)):
        idx = fi_ + 4 * si + mi
        seed, off = RNGS[idx % len(RNGS)]
        p = (0.5, 0.6, 0.17)[idx % 3]
        q, k = (torch.randn(B, s, h, d, generator=g).to(device=DEV, dtype=torch.bfloat16) for s, h in ((sq, H), (sk, HK)))
        set_generator(seed, off)
        _, _, rv, rng = be.fwd(q, k, k, None, _alibi(alibi, B), p, dp.SCALE, mask[0], mask[1], mask[2], cap, True, None)
        s = be.last_schedule()
        assert s["fwd_kernel"] == 1 and (d not in (64, 128) or s["fwd_nw"] == nw), s
        assert rng.tolist() == [seed, off]
        vis = mp.visible(sq, sk, mask, None, DEV)
        for b in range(B):
            _check_payload(rv[b], vis, dp.model_bytes(seed, off, H, b, sq, sk, DEV), "%s Sq %d Sk %d mask %s batch %d" % (feature, sq, sk, mp.mask_name(mask), b))


@pytest.mark.parametrize("d", [64, 128])
def test_payload_equals_model_packed(be, knobs, d):
    """fa_varlen_fwd: payload (H, total_q, max_seqlen_k); rows and keys count from 0 in each sequence and b is the sequence's index."""
    seqs = packed_seqs()
    lq, lk = [s[0] for s in seqs], [s[1] for s in seqs]
    cu_q = torch.tensor([0] + list(np.cumsum(lq)), dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([0] + list(np.cumsum(lk)), dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(d)
    q = torch.randn(sum(lq), H, d, generator=g).to(device=DEV, dtype=torch.bfloat16)
    k = torch.randn(sum(lk), HK, d, generator=g).to(device=DEV, dtype=torch.bfloat16)
    for idx, mask in enumerate(MASKS):
        seed, off = RNGS[idx % len(RNGS)]
        set_generator(seed, off)
        _, _, rv, rng = be.varlen_fwd(q, k, k, None, cu_q, cu_k, None, None, None, None, max(lq), max(lk), 0.5, dp.SCALE, False, mask[0], mask[1], mask[2], 0.0, True, None)
        assert rng.tolist() == [seed, off] and tuple(rv.shape) == (H, sum(lq), max(lk))
        for b, (nq, nk) in enumerate(seqs):
            if nq:
                r0 = int(cu_q[b])
                _check_payload(rv[:, r0:r0 + nq, :nk], mp.visible(nq, nk, mask, max(lk), DEV), dp.model_bytes(seed, off, H, b, nq, nk, DEV),
                               "packed entry %d mask %s" % (b, mp.mask_name(mask)))
                assert int(rv[:, r0:r0 + nq, nk:].sum()) == 0, "no byte is written behind a sequence's last key"


# ---------------------------------------------------------------- b. / c. every pinned kernel ----------------------------------------------------------------
def groups(side):
    """{(dt, head dim): [pinned rows with keys on that side]}: one test per group, every row of it pinned, probed and proven from the launch log in turn."""
    out = {}
    for r in PINNED:
        if r[side]:
            out.setdefault((r["dt"], r["d"]), []).append(r)
    return out


def _forward_row(be, knobs, row):
    w64 = any(k[0] == "fa_fwd_w64_kernel" for k in row["fwd_keys"])
    run = Run(be, knobs, {k: v for k, v in row["knobs"].items() if k.startswith("FA_FWD") or k.startswith("FA_IL")}, family_label(row))
    dtype = DT[row["dt"]]
    for idx, (shape, mask, p, rng) in enumerate(schedule(row)):
        for persist in ((1, 0) if w64 and shape == SHAPES[2] else (None,)):
            if persist is not None:
                knobs.set("FA_W64_PERSIST", persist)
            probe_forward(run, problem(shape, mask, p, rng, row["d"], dtype), row["cap"], row["alibi"], return_softmax=(not w64 and idx % 2 == 1),
                          extra="" if persist is None else " persist=%d" % persist)
    if w64:
        for mask, persist in itertools.product(MASKS[:2], (1, 0)):
            knobs.set("FA_W64_PERSIST", persist)
            probe_forward(run, problem(None, mask, 0.5, RNGS[0], row["d"], dtype, packed_tiles=1), packed=True, extra=" packed persist=%d" % persist)
    run.assert_ran(row["fwd_keys"])
    run.close()


@pytest.mark.parametrize("dt,d", sorted(groups("fwd_keys")))
def test_forward_probe(be, knobs, dt, d):
    """Every mask-drawing forward key of this dtype and head dim: the lock-step variants with and without return_softmax (the same kernel, the payload store
    on and off), the 64-rows-per-wave kernel dense and packed with the persistent walk on and off."""
    for row in groups("fwd_keys")[(dt, d)]:
        _forward_row(be, knobs, row)


@pytest.mark.parametrize("dt,d", sorted(groups("bwd_keys")))
def test_backward_probe(be, knobs, dt, d):
    """Every mask-drawing dQ and dK/dV key of this dtype and head dim (4 and 8 waves, the 64-rows-per-wave dQ kernel): the dV probe, then the dQ probe,
    rng_state written by the test."""
    for row in groups("bwd_keys")[(dt, d)]:
        kn = {k: v for k, v in row["knobs"].items() if not k.startswith("FA_FWD")}
        assert kn.get("FA_BWD_MODE") == 1 and kn.get("FA_BWD_GSPLIT") == 0, kn
        run = Run(be, knobs, kn, family_label(row))
        for shape, mask, p, rng in schedule(row):
            probe_backward(run, problem(shape, mask, p, rng, row["d"], DT[row["dt"]]), row["cap"], row["alibi"])
        run.assert_ran(row["bwd_keys"])
        run.close()


@pytest.mark.parametrize("p", OTHER_P)
def test_other_dropout_rates(be, knobs, p):
    """p = 0.17, 0.6 (where the single-precision threshold, 101, is not the double-precision 102), 0.999 (threshold 0) and 0.001 (254) on one kernel per family:
    the 8-wave lock-step forward, the 64-rows-per-wave forward, the 8-wave dQ + dK/dV pair and the 64-rows-per-wave dQ kernel, D = 128, none and causal."""
    assert (p, dm.threshold(p)) in ((0.17, 211), (0.6, 101), (0.999, 0), (0.001, 254))
    for nw in (8, 64):
        run = Run(be, knobs, {"FA_FWD_NW": nw}, "other p: fwd nw=%d" % nw)
        for mask in MASKS[:2]:
            probe_forward(run, problem(SHAPES[2], mask, p, RNGS[0], 128, torch.bfloat16))
        run.assert_ran([kc.K("fa_fwd_kernel", "bf16", 128, 128, 8, kc.DROP, False) if nw == 8 else kc.K("fa_fwd_w64_kernel", "bf16", 128, kc.DROP, False, False)])
    for dq_nw, key in ((8, kc.K("fa_bwd_dq_kernel", "bf16", 128, 128, 8, kc.DROP, 128)), (64, kc.K("fa_bwd_dq_w64_kernel", "bf16", 128, True, kc.DROP))):
        run = Run(be, knobs, dict(kc.PAIR_OFF, FA_BWD_DQ_NW=dq_nw, FA_BWD_DKDV=8 if dq_nw == 8 else 64), "other p: bwd dq_nw=%d" % dq_nw)
        for mask in MASKS[:2]:
            probe_backward(run, problem(SHAPES[2], mask, p, RNGS[0], 128, torch.bfloat16))
        run.assert_ran([key, kc.K("fa_bwd_dkdv_kernel", "bf16", 128, 128, kc.DROP, 128)])


@pytest.mark.parametrize("work_list", [1, 0])
@pytest.mark.parametrize("d", [64, 128])
def test_packed_backward(be, knobs, d, work_list):
    """varlen_bwd over the packed batch six times over, with the query-block and key-block work lists (bwd_list = 3) and with FA_VARLEN_LIST=0."""
    run = Run(be, knobs, dict(kc.PAIR_OFF, FA_VARLEN_LIST=work_list), "varlen_bwd d%d list=%d" % (d, work_list))
    for idx, mask in enumerate(MASKS):
        probe_backward(run, problem(None, mask, 0.5, RNGS[idx % len(RNGS)], d, torch.bfloat16, packed_tiles=PACKED_TILES), packed=True, extra=" packed")
        assert bool(be.last_schedule()["bwd_list"]) == bool(work_list), be.last_schedule()


@pytest.mark.parametrize("d", [64, 128])
def test_default_dispatch(be, knobs, d):
    """No schedule knobs: whatever the tables pick on the census shape and on (300, 1100) must keep the model's pairs, forward and backward."""
    for name in ("FA_FWD_NW", "FA_BWD_DQ_NW", "FA_BWD_DKDV", "FA_BWD_MODE", "FA_BWD_GSPLIT", "FA_STRICT", "FA_PACK_GQA", "FA_VARLEN_LIST", "FA_W64_PERSIST"):
        knobs.unset(name)
    run = Run(be, knobs, {}, "default dispatch d%d" % d)
    for idx, (shape, mask) in enumerate(itertools.product((SHAPES[2], BIG), MASKS)):
        pb = problem(shape, mask, 0.5, RNGS[3] if shape == BIG else RNGS[idx % len(RNGS)], d, torch.bfloat16)
        probe_forward(run, pb, extra=" default")
        pl = plan_of(pb)
        probe_backward(run, pb, extra=" default plan=%d gsplit=%d" % (pl[0], pl[3]), dv_threshold=dp.THRESHOLD_SPLIT if pl[3] else dp.THRESHOLD)
    assert any(k and k[0] in MASK_FAMILIES[:2] and draws_mask(k) for k in run.ran) and any(k and k[0] in MASK_FAMILIES[2:] and draws_mask(k) for k in run.ran), run.ran


# ---------------------------------------------------------------- d. the GQA group split ----------------------------------------------------------------
def plan_of(pb):
    """fa_bwd_plan_query of the fixed-length call: out[0] = launch kind (0 = the dQ + dK/dV pair), out[3] = virtual kv heads a GQA group is split into (0 = unsplit)."""
    import ctypes as C
    from flash_attn_amd import _cabi
    a = _cabi.FaBwdParams()
    a.b, a.h, a.h_k, a.d = len(pb.seqs), pb.h, pb.hk, pb.d
    a.seqlen_q, a.seqlen_k, a.total_q, a.total_k = pb.seqs[0][0], pb.seqs[0][1], len(pb.seqs) * pb.seqs[0][0], len(pb.seqs) * pb.seqs[0][1]
    a.dtype = _cabi.FA_DTYPE_BF16 if pb.dtype == torch.bfloat16 else _cabi.FA_DTYPE_FP16
    a.softmax_scale, a.is_causal, a.window_left, a.window_right = dp.SCALE, int(pb.mask[0]), pb.mask[1], pb.mask[2]
    a.p_dropout = float(pb.p)
    out = (C.c_int32 * 8)()
    assert _cabi.load().fa_bwd_plan_query(C.byref(a), out, 8) == 8
    return list(out)


@pytest.mark.parametrize("gsplit", [16, None], ids=["forced", "automatic"])
def test_group_split(be, knobs, monkeypatch, gsplit):
    """FA_BWD_GSPLIT=16 (forced) and unset (automatic): every virtual kv head of a split group must draw the stream of its QUERY heads.  Booked under what
    fa_bwd_plan_query reports; a forced run must have split (a workspace for every call) and its dV is held to THRESHOLD_SPLIT (tests/_dropout_probe.py)."""
    kn = {"FA_BWD_MODE": 1, "FA_BWD_DQ_NW": 8, "FA_BWD_DKDV": 8}
    if gsplit is not None:
        kn["FA_BWD_GSPLIT"] = gsplit
    else:
        knobs.unset("FA_BWD_GSPLIT")
    run = Run(be, knobs, kn, "group split %s" % ("forced" if gsplit else "automatic"))
    allocs, real = [], be._alloc_workspace
    monkeypatch.setattr(be, "_alloc_workspace", lambda n, dev: (allocs.append(n), real(n, dev))[1])
    split_cases = 0
    for idx, ((shape, mask), (h, hk)) in enumerate(itertools.product(itertools.product(SHAPES, MASKS), ((4, 2), (8, 1)))):
        pb = dp.Problem([shape] * B, mask, 0.5, RNGS[idx % len(RNGS)], h, hk, 128, 128, torch.bfloat16, DEV)
        pl = plan_of(pb)
        split_cases += bool(pl[3])
        before = len(allocs)
        probe_backward(run, pb, extra=" H %d/%d plan=%d gsplit=%d" % (h, hk, pl[0], pl[3]), dv_threshold=dp.THRESHOLD_SPLIT if pl[3] else dp.THRESHOLD)
        assert (len(allocs) > before) == bool(pl[3]), "a split call takes a workspace, an unsplit one does not: plan %s" % pl
    if gsplit:
        assert split_cases == 2 * len(SHAPES) * len(MASKS), split_cases
        assert any(k and k[0] == "fa_bwd_gsum_kernel" for k in run.ran), sorted(kc.key_str(k) for k in run.ran if k)


# ---------------------------------------------------------------- e. the public functions ----------------------------------------------------------------
def _public_round_trip(fn_call, seqs, mask, p, d, max_k=None, label=""):
    """fn_call(q_e, k_e, v_e, dout_e or None) -> (out_e, lse_e, rng_state, dv_e or None): forward probe from out / lse, then the dV probe through autograd.grad."""
    # forward: V codes, q = 0; the keep set is known only once the call has returned its rng_state, so the decoding follows the call
    seqs = list(seqs)
    codes = [mp.fwd_codes(nk, d, DEV) for _, nk in seqs]
    assert all(c.shape[0] == 1 for c in codes), "one pass"
    q_e = [torch.zeros(nq, H, d, device=DEV, dtype=torch.bfloat16) for nq, _ in seqs]
    k_e = [dp.rand_k((nk, HK, d), torch.bfloat16, DEV) for _, nk in seqs]
    v_e = [c[0][:, None, :].expand(-1, HK, -1).contiguous().to(torch.bfloat16) for c in codes]
    out_e, lse_e, rng, _ = fn_call(q_e, k_e, v_e, None)
    seed, off = [x & ((1 << 64) - 1) for x in rng.tolist()]
    pb = dp.Problem(seqs, mask, p, (seed, off), H, HK, d, d, torch.bfloat16, DEV, max_k=max_k)
    run = _PublicRun(label)
    run.finish(dp.probe_fwd(pb, lambda *_: list(zip(out_e, lse_e))), "forward through autograd", torch.bfloat16)
    # dV: v = 0, coded dO; the call draws a new rng_state, so the expected set is built after it
    pr = [dp._dv_codes(nq, nk, tuple(mask), max_k, d, H // HK, p, DEV) for nq, nk in seqs]
    assert all(c[0].shape[0] == 1 for c in pr), "one pass"
    do_e = [c[0][0][None].expand(HK, -1, -1, -1).reshape(H, nq, d).permute(1, 0, 2).contiguous().to(torch.bfloat16) for c, (nq, _) in zip(pr, seqs)]
    z_e = [torch.zeros_like(v) for v in v_e]
    _, _, rng2, dv_e = fn_call(q_e, k_e, z_e, do_e)
    seed2, off2 = [x & ((1 << 64) - 1) for x in rng2.tolist()]
    assert (seed2, off2) != (seed, off), "the generator's offset advances between calls"
    pb2 = dp.Problem(seqs, mask, p, (seed2, off2), H, HK, d, d, torch.bfloat16, DEV, max_k=max_k)
    run.finish(dp.probe_dv(pb2, lambda *_: [(torch.zeros(()), torch.zeros(()), g) for g in dv_e]), "dV through autograd.grad", torch.bfloat16)


class _PublicRun(Run):
    def __init__(self, label):
        self.label, self.ran = label, {}


def test_flash_attn_func_under_autograd():
    from flash_attn_amd import flash_attn_interface as fi
    (sq, sk), mask, p, d = SHAPES[2], MASKS[1], 0.5, 128

    def call(q_e, k_e, v_e, do_e):
        q, k, v = (torch.stack(t).requires_grad_() for t in (q_e, k_e, v_e))
        out, lse, _ = fi.flash_attn_func(q, k, v, dropout_p=p, softmax_scale=dp.SCALE, causal=True, return_attn_probs=True)
        rng = out.grad_fn.saved_tensors[5]
        dv = None if do_e is None else list(torch.autograd.grad(out, v, torch.stack(do_e))[0])
        return list(out.detach()), list(lse), rng, dv
    _public_round_trip(call, [(sq, sk)] * B, mask, p, d, label="flash_attn_func")


def test_flash_attn_varlen_func_under_autograd():
    from flash_attn_amd import flash_attn_interface as fi
    seqs, mask, p, d = packed_seqs(), MASKS[1], 0.5, 128
    lq, lk = [s[0] for s in seqs], [s[1] for s in seqs]
    cu_q = torch.tensor([0] + list(np.cumsum(lq)), dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([0] + list(np.cumsum(lk)), dtype=torch.int32, device=DEV)
    cq, ck = cu_q.tolist(), cu_k.tolist()

    def call(q_e, k_e, v_e, do_e):
        q, k, v = (torch.cat(t).requires_grad_() for t in (q_e, k_e, v_e))
        out, lse, _ = fi.flash_attn_varlen_func(q, k, v, cu_q, cu_k, max(lq), max(lk), dropout_p=p, softmax_scale=dp.SCALE, causal=True, return_attn_probs=True)
        rng = [t for t in out.grad_fn.saved_tensors if t.dtype == torch.int64 and t.numel() == 2][0]
        dv = None
        if do_e is not None:
            g = torch.autograd.grad(out, v, torch.cat(do_e))[0]
            dv = [g[ck[b]:ck[b + 1]] for b in range(len(seqs))]
        return [out.detach()[cq[b]:cq[b + 1]] for b in range(len(seqs))], [lse[:, cq[b]:cq[b + 1]] for b in range(len(seqs))], rng, dv
    _public_round_trip(call, seqs, mask, p, d, max_k=max(lk), label="flash_attn_varlen_func")


def test_flash_attn_padded_func_under_autograd():
    """A padded batch (B, S, H, D) whose seqused_q / seqused_k shorten two entries: each entry is a sequence of its own used lengths."""
    from flash_attn_amd import flash_attn_interface as fi
    sq, sk, mask, p, d = 293, 331, MASKS[1], 0.5, 128
    used_q, used_k = [293, 120, 293, 65], [331, 331, 130, 77]
    seqs = list(zip(used_q, used_k))
    lens_q = torch.tensor(used_q, dtype=torch.int32, device=DEV)
    lens_k = torch.tensor(used_k, dtype=torch.int32, device=DEV)

    def pad(ts, rows, fill):
        return torch.stack([torch.cat([t, torch.full((rows - t.shape[0],) + tuple(t.shape[1:]), fill, device=DEV, dtype=t.dtype)]) for t in ts])

    def call(q_e, k_e, v_e, do_e):
        q, k, v = pad(q_e, sq, 0.0).requires_grad_(), pad(k_e, sk, 1.0).requires_grad_(), pad(v_e, sk, 3.0).requires_grad_()
        out = fi.flash_attn_padded_func(q, k, v, lens_q, lens_k, dropout_p=p, softmax_scale=dp.SCALE, causal=True)
        saved = out.grad_fn.saved_tensors
        rng = [t for t in saved if t.dtype == torch.int64 and t.numel() == 2][0]
        lse = [t for t in saved if t.dtype == torch.float32 and t.dim() == 2][0]          # (H, total_q) of the flattened batch
        dv = None
        if do_e is not None:
            g = torch.autograd.grad(out, v, pad(do_e, sq, 0.0))[0]
            dv = [g[b, :used_k[b]] for b in range(len(seqs))]
        return [out.detach()[b, :used_q[b]] for b in range(len(seqs))], [lse[:, b * sq:b * sq + used_q[b]] for b in range(len(seqs))], rng, dv
    _public_round_trip(call, seqs, mask, p, d, max_k=sk, label="flash_attn_padded_func")


# ---------------------------------------------------------------- the probe can fail here too ----------------------------------------------------------------
@pytest.mark.parametrize("wrong", ["offset+4", "seed_high_cleared", "fp64_threshold_at_0.6"])
def test_a_kernel_drawing_another_keep_set_is_reported(be, knobs, wrong):
    """The decoders expect a keep set that is NOT the one the kernels draw -- the stream of another offset, of a seed without its high word, and at p = 0.6
    the double-precision threshold 102 where the library's is 101 (one byte value in 256) -- and the forward, the dV and the dQ probe must each report it, with
    the batch, head and row in the message (tests/test_dropout_probe_cpu.py does this to a stand-in with thirteen wrong sets).  Nothing of this is recorded."""
    run = Run(be, knobs, dict(kc.PAIR_OFF, FA_FWD_NW=8, FA_BWD_DQ_NW=8, FA_BWD_DKDV=8), "self-test")
    seed, off = RNGS[0]
    p = 0.6 if wrong.startswith("fp64") else 0.5
    given = problem(SHAPES[1], MASKS[1], p, (seed, off), 128, torch.bfloat16)
    expected = problem(SHAPES[1], MASKS[1], p, {"offset+4": (seed, off + 4), "seed_high_cleared": (seed & 0xFFFFFFFF, off)}.get(wrong, (seed, off)), 128, torch.bfloat16)
    if wrong.startswith("fp64"):
        expected.keep = [dp.model_bytes(seed, off, H, b, *SHAPES[1], DEV) <= 102 for b in range(B)]
    fwd, bwd = calls(run, given)
    saved = dict(_MARGINS)
    try:
        for probe, call, pattern in ((dp.probe_fwd, fwd, r"identity: batch \d+ head \d+ row \d+"), (dp.probe_dv, bwd, r"dV: batch \d+ kv head \d+ key \d+"),
                                     (dp.probe_dq, bwd, r"dQ: batch \d+ head \d+ row \d+")):
            with pytest.raises(pytest.fail.Exception, match=pattern):
                run.finish(probe(expected, call), wrong, torch.bfloat16)
    finally:
        _MARGINS.clear()
        _MARGINS.update(saved)
