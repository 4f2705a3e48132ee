"""The dropout probe (tests/_dropout_probe.py, tests/_dropout_model.py) can fail, and its kernel list is complete.  No GPU.

  * the model: the numpy implementation of hash32 / bh_key / drop_bytes against the same on Python ints with explicit masks, on a few thousand random
    (seed, offset, bh, i, g) with bits above 2^32 in seed and offset and i, g up to 2^20 (a guard of numpy's wrap-around and promotion rules, not of the
    kernels); the single-precision threshold, which differs from Python's double-precision one at exactly p = 0.6 over p = k/100, k/256, k/1000;
  * the stand-in: a torch attention with dropout and the kernels' roundings (P and dS rounded to the dtype, fp32 sums, outputs rounded once), run over EVERY
    numeric case of the GPU module (tests/test_dropout_probe_gpu.py numeric_cases(): shape x mask x p x rng x head dim x dtype), stays within HALF the
    threshold on all three decoders with the model's keep set;
  * the mutants: with each of thirteen wrong keep sets the stand-in is reported by the forward, the dV and the dQ decoder, in a (batch, head, row) that really
    differs, on the first cases where the mutant is live; the number of numeric cases in which each mutant is live is asserted (LIVE);
  * coverage: the GPU module's list of pinned kernels holds every census key that can draw a mask, with no exclusion list."""
import math
import random

import numpy as np
import pytest
import torch

from tests import _dropout_model as dm
from tests import _dropout_probe as dp
from tests import _kernel_census as kc
from tests import _mask_probe as mp
from tests import test_dropout_probe_gpu as gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
CASES = gpu.numeric_cases()


# ---------------------------------------------------------------- the model ----------------------------------------------------------------
def test_numpy_model_equals_the_scalar_model():
    rnd = random.Random(5)
    n = 4000
    seeds = [rnd.getrandbits(64) if t % 2 else rnd.getrandbits(31) for t in range(n)]
    offs = [rnd.getrandbits(64) if t % 3 else rnd.getrandbits(20) * 4 for t in range(n)]
    bhs = [rnd.getrandbits(rnd.choice((3, 8, 16, 31))) for _ in range(n)]
    rows = [rnd.getrandbits(rnd.choice((4, 10, 20))) for _ in range(n)]
    grps = [rnd.getrandbits(rnd.choice((4, 10, 20))) for _ in range(n)]
    assert max(rows) >= 1 << 19 and max(grps) >= 1 << 19 and max(seeds) >= 1 << 63 and max(offs) >= 1 << 63
    xs = [rnd.getrandbits(32) for _ in range(n)]
    assert dm.hash32(np.array(xs, dtype=np.uint64)).tolist() == [dm.hash32_int(x) for x in xs]
    keys = dm.bh_key(seeds, offs, np.array(bhs, dtype=np.uint64))
    assert keys.tolist() == [dm.bh_key_int(s, o, b) for s, o, b in zip(seeds, offs, bhs)]
    words = dm.drop_bytes(keys, np.array(rows, dtype=np.uint64), np.array(grps, dtype=np.uint64))
    assert words.tolist() == [dm.drop_bytes_int(k, i, g) for k, i, g in zip(keys.tolist(), rows, grps)]
    assert int(words.max()) < 1 << 32 and len(set(words.tolist())) > n - 3
    # a negative int64 (what an rng_state tensor holds for a seed >= 2^63) is its two's complement
    assert dm.bh_key(-5, -9, 3).tolist() == dm.bh_key_int((1 << 64) - 5, (1 << 64) - 9, 3) == dm.bh_key_int(-5, -9, 3)


def test_rand_bytes_layout():
    """rand_bytes is pair_byte over (b * H + h, i, j): byte j & 3 of the word of group j >> 2; a packed sequence is entry b of its own lengths."""
    seed, off = gpu.RNGS[0]
    rb = dm.rand_bytes(seed, off, 2, 3, 5, 11)
    for b, h, i, j in ((0, 0, 0, 0), (1, 2, 4, 10), (1, 0, 3, 7), (0, 2, 1, 5)):
        w = dm.drop_bytes_int(dm.bh_key_int(seed, off, b * 3 + h), i, j >> 2)
        assert int(rb[b, h, i, j]) == (w >> (8 * (j & 3))) & 0xFF
    keys = dm.bh_key(seed, off, np.arange(6, dtype=np.uint64).reshape(2, 3))[:, :, None, None]
    assert np.array_equal(rb, dm.pair_byte(keys, np.arange(5, dtype=np.uint64)[None, None, :, None], np.arange(11, dtype=np.uint64)[None, None, None, :]))
    assert np.array_equal(dm.rand_bytes(seed, off, 1, 3, 4, 9, b0=1)[0], rb[1, :, :4, :9])
    kp = dm.keep_packed(seed, off, 0.5, 3, [5, 4], [11, 9])
    assert np.array_equal(kp[1], rb[1, :, :4, :9] <= 127) and np.array_equal(kp[0], rb[0] <= 127)


def test_threshold_is_single_precision():
    assert dm.threshold(0.6) == 101 and math.floor(255.0 * (1.0 - 0.6)) == 102
    assert (dm.threshold(0.5), dm.threshold(0.17), dm.threshold(0.999), dm.threshold(0.001), dm.threshold(0.0)) == (127, 211, 0, 254, 255)
    ps = sorted({k / 100 for k in range(100)} | {k / 256 for k in range(256)} | {k / 1000 for k in range(1000)})
    assert [p for p in ps if dm.threshold(p) != math.floor(255.0 * (1.0 - p))] == [0.6]


def test_scales_and_caps():
    assert [(dp.scale_pow2(p), dp.cap_for(p)) for p in (0.5, 0.17, 0.6, 0.999, 0.001)] == [(0.5, 16), (1.0, 13), (0.5, 12), (2.0 ** -10, 16), (1.0, 15)]
    for p in (0.5, 0.17, 0.6, 0.999, 0.001):
        assert 0.97 < dp.scale_pow2(p) / dm.p_keep(p) < 1.2501 and dp.cap_for(p) * dp.term_max(p) <= dp.SUM_BOUND   # a flipped pair moves >= 0.97; sum of |terms| <= 32


# ---------------------------------------------------------------- the stand-in over the GPU module's cases ----------------------------------------------------------------
def _problem(case):
    packed, shape, mask, p, rng, d, dt = case
    if packed:
        seqs = gpu.packed_seqs()
        return dp.Problem(seqs, mask, p, rng, gpu.H, gpu.HK, d, d, DT[dt], "cpu", max_k=max(s[1] for s in seqs)), seqs
    return dp.Problem([shape] * gpu.B, mask, p, rng, gpu.H, gpu.HK, d, d, DT[dt], "cpu"), None


def _run_all(pb, keep=None):
    fwd, bwd = dp.standin_calls(pb, keep)
    return {"fwd": dp.probe_fwd(pb, fwd, dp.assert_uniform_scores), "dv": dp.probe_dv(pb, bwd, dp.assert_uniform_scores), "dq": dp.probe_dq(pb, bwd)}


_WORST = {}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-p%g-d%d-%s" % ("packed" if c[0] else "%dx%d" % c[1], mp.mask_name(c[2]), c[3], c[5], c[6]))
def test_standin_with_the_model_keep_set_is_within_half_the_threshold(case):
    pb, _ = _problem(case)
    for name, res in _run_all(pb).items():
        worst, exact = res.worst()
        assert exact == 0, (name, [(int(c), w) for c, w in res.zeros if int(c)])
        for dec, v in worst.items():
            key = (dec, case[6])
            _WORST[key] = max(_WORST.get(key, 0.0), v)
            assert v <= dp.THRESHOLD / 2, (name, dec, v)


def test_standin_worst_deviations_are_reported():
    """(Runs after the cases above: prints what profiles/dropout_probe_margins.txt records.)"""
    print("stand-in worst deviations:", {k: round(v, 4) for k, v in sorted(_WORST.items())})
    assert not _WORST or max(_WORST.values()) <= dp.THRESHOLD / 2


# ---------------------------------------------------------------- the mutants ----------------------------------------------------------------
# the number of numeric cases in which each mutant differs from the model on a visible pair (asserted: a list too narrow for a mutant shows here)
N_CASES, N_PACKED = len(CASES), sum(1 for c in CASES if c[0])
N_ROW256 = sum(1 for c in CASES if c[0] or c[1][0] > 256)
N_OFF_HIGH = sum(1 for c in CASES if c[4][1] >= 1 << 32)
N_SEED_HIGH = sum(1 for c in CASES if c[4][0] >= 1 << 32)
N_P06 = sum(1 for c in CASES if c[3] == 0.6)
LIVE = {"bytes_reversed": N_CASES, "group_tile_local": N_CASES, "group_bottom_right": N_CASES, "row_block_local": N_ROW256, "packed_global_row_key": N_PACKED,
        "packed_b0": N_PACKED, "kv_head": N_CASES, "bh_hk": N_CASES, "counter_swapped": N_CASES, "strict_less": N_CASES, "offset_high_ignored": N_OFF_HIGH,
        "seed_high_ignored": N_SEED_HIGH, "fp64_threshold": N_P06}
RUN_PER_MUTANT = 2   # the stand-in runs on the first two live cases of each mutant (smallest first); liveness is counted over all of them


def _cu(seqs):
    return [0] + list(np.cumsum([s[0] for s in seqs])), [0] + list(np.cumsum([s[1] for s in seqs]))


def _differs(pb, mut, b, h, rows, key=None, group=False):
    heads = range(h * pb.ratio, (h + 1) * pb.ratio) if group else (h,)
    for hh in heads:
        d = (mut[b][hh] != pb.keep[b][hh]) & pb.vis[b]
        if key is not None:
            if bool(d[rows, key].any()):
                return True
        elif bool(d[rows].any()):
            return True
    return False


@pytest.mark.parametrize("name", dp.MUTANTS)
def test_every_mutant_is_reported_by_every_decoder(name):
    assert min(N_PACKED, N_ROW256, N_OFF_HIGH, N_SEED_HIGH, N_P06) >= 2 and N_ROW256 < N_CASES and N_OFF_HIGH < N_CASES
    live = []
    for case in CASES:
        pb, seqs = _problem(case)
        cu_q, cu_k = _cu(seqs) if seqs else (None, None)
        mut = dp.mutant_keep(name, pb, cu_q, cu_k)
        if mut is not None:
            live.append((case, pb, mut))
    assert len(live) == LIVE[name], (name, len(live), LIVE[name])
    live.sort(key=lambda t: (sum(nq * nk for nq, nk in t[1].seqs), repr(t[0])))
    for case, pb, mut in live[:RUN_PER_MUTANT]:
        res = _run_all(pb, mut)
        for dec, group in (("fwd", False), ("dv", True), ("dq", False)):
            worst, _ = res[dec].worst()
            assert max(worst[d] for d in worst if d != "count") >= dp.THRESHOLD, (name, dec, case, worst)
            assert dec != "fwd" or worst["count"] <= dp.THRESHOLD / 2, "lse is that of the un-dropped scores: a wrong keep set leaves the count alone"
            fails = [f for _, v, ex in res[dec].devs if ex is not None and not float(v) < dp.THRESHOLD for f in ex()]
            assert fails, (name, dec)
            for msg, b, h, rows, key, _ in fails[:12]:
                assert ("too high" in msg) or ("too low" in msg), msg
                assert _differs(pb, mut, b, h, rows, key, group), (name, dec, msg)


# ---------------------------------------------------------------- coverage ----------------------------------------------------------------
def test_the_pinned_list_covers_every_mask_drawing_key_of_the_census():
    """Every census key of the five families whose feature code has the DROP bit (FEAT_ALL included) is pinned by a GPU test that asserts, from the launch log,
    that it ran under no mask and under the causal mask.  No exclusion list."""
    need = set()
    for r in kc.RECIPES:
        for family, dtype, args in r["keys"]:
            if family in ("fa_fwd_kernel", "fa_fwd_w64_kernel", "fa_bwd_dq_kernel", "fa_bwd_dkdv_kernel", "fa_bwd_dq_w64_kernel"):
                feat = args[{"fa_fwd_kernel": 3, "fa_fwd_w64_kernel": 1, "fa_bwd_dq_kernel": 3, "fa_bwd_dkdv_kernel": 2, "fa_bwd_dq_w64_kernel": 2}[family]]
                if feat in (kc.DROP, kc.CAP | kc.DROP, kc.ALIBI | kc.DROP, kc.ALL):
                    need.add((family, dtype, args))
    have_f = {k for row in gpu.PINNED for k in row["fwd_keys"]}
    have_b = {k for row in gpu.PINNED for k in row["bwd_keys"]}
    assert need == have_f | have_b, sorted(kc.key_str(k) for k in need ^ (have_f | have_b))
    assert len(need) >= 130 and {k[0] for k in need} == set(gpu.MASK_FAMILIES)
    # no other family of the census carries a feature code at all next to these: every family with "DROP" reachable is one of the five
    assert all(k[0].startswith("fa_fwd") for k in have_f) and all(k[0].startswith("fa_bwd") for k in have_b)
    # every pinned row is parametrised into the GPU test of its side, and every schedule holds the no-mask and the causal case
    for row in gpu.PINNED:
        masks = {mp.mask_name(m) for _, m, _, _ in gpu.schedule(row)}
        assert {"none", "causal"} <= masks, row["id"]
        if row["bwd_keys"]:
            assert row["knobs"].get("FA_BWD_MODE") == 1 and row["knobs"].get("FA_BWD_GSPLIT") == 0, row["id"]
    # the kernels that refuse dropout have no such key: the fused / chunked launches, the 64-per-wave dK/dV kernel, the (192, 128) pair
    for family in ("fa_bwd_fused_kernel", "fa_bwd_c5_kernel", "fa_fwd_dv_kernel", "fa_fwd_il_kernel"):
        assert not any(k[0] == family for k in need)
