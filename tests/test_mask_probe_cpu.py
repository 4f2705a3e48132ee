"""The mask probe (tests/_mask_probe.py) can fail: on the CPU, with a plain torch attention that rounds P / dS and the outputs to the dtype standing in for the
kernels, the correct masks pass with a deviation of at most 0.15 and every wrong mask of _mask_probe.MUTANTS is reported by at least one decoder, in a row where
the wrong mask differs from the right one.  The forward decoders see every mutant first; test_backward_decoders_report_on_their_own runs the dV and the dQ
decoder without them.

Cases: the probe's shape list x its mask list ("fixed"), the KV-cache shapes (Sq x cache_seqlens x the cache path's masks, "cache") and the sequences of the packed
batch (plain and with seqused_k, "packed"), in bf16 and fp16, at head dim 64 and 128, with group ratios 1, 2 and 4 (4 and 8 on the cache shapes) chosen from
shape + mask, so that a mask meets every ratio.  A mutant is skipped only where it provably equals the correct mask (mutant_mask returns None, or the two masks
are equal); each must be LIVE in at least one third of the cases of its domain:
  wr+-1, wl+-1, top_left, seam_tile, last_key   all fixed cases
  row_mod_sq, row_div_g   all fixed cases and all cache cases (not live at ratio 1 or with one query row: r % Sq == r // g)
  masked_row_key    the fixed and cache cases with Sq > Sk >= 1: with Sq <= Sk the last row sees the last key under every mask of the lists, no row is empty, and
                    the mutant is live in 18 of the 120 fixed cases
  own_sk            the packed batch with seqused_k = [40, 65, 5, 300, 77, 10], one case per mask: a bound normalised by a sequence's own Sk differs from the
                    one normalised by max_seqlen_k only where Sk <= wr < Sq - 1 (a left bound >= Sk hides nothing either way): in none of the fixed cases, and
                    on the plain batch for (255, 256) alone -- that case is run and must be caught too, but the share is taken over the shortened batch."""
import itertools

import pytest
import torch

from tests import _mask_probe as mp

DTYPES = [torch.bfloat16, torch.float16]
PASS_BOUND = 0.15


def _heads(vis_or_wrong, hk, ratio):
    """A wrong mask per query head of a group (g, Sq, Sk) -> (H, Sq, Sk); a plain one stays."""
    return vis_or_wrong.repeat(hk, 1, 1) if vis_or_wrong.dim() == 3 else vis_or_wrong


def run_probe(sq, sk, mask, max_k, dtype, d, hk, ratio, wrong=None, first_only=False, decoders=("fwd", "dv", "dq")):
    """The decoders on the stand-in, one sequence.  -> ({decoder: worst deviation}, exact violations, [(message, head, rows)])."""
    torch.manual_seed(sq * 131 + sk)
    vis = mp.visible(sq, sk, mask, max_k)
    used = vis if wrong is None else _heads(wrong, hk, ratio)
    h = hk * ratio
    devs, exact, fails = {}, 0, []
    q = torch.zeros(sq, h, d, dtype=dtype)
    krand = torch.randn(sk, hk, d).to(dtype)

    def worst(name, x):
        devs[name] = max(devs.get(name, 0.0), float(x))

    codes = mp.fwd_codes(sk, d)
    exp = mp.fwd_expected(vis, codes)
    for call in range(mp.n_calls(codes.shape[0], hk) if "fwd" in decoders else 0):
        po = mp.slot_passes(codes.shape[0], 1, hk, call)
        v = mp.fwd_values(codes, po, dtype)[0]
        out, lse = mp.standin_fwd(q, krand, v, used)
        poh = po[0].repeat_interleave(ratio)
        r = mp.fwd_check(out, lse, vis, exp, poh)
        for nm in ("count", "fine", "coarse"):
            worst("fwd_" + nm, r[nm])
        exact += int(r["exact"])
        if wrong is not None:
            fails += mp.fwd_failures(out, lse, vis, exp, poh)
    if first_only and fails:
        return devs, exact, fails
    lse_ref = mp.ref_lse(vis)[None].expand(h, -1)
    do_codes, exp_dv = mp.dv_probe(sq, sk, mask, d, ratio, max_k)
    for call in range(mp.n_calls(do_codes.shape[0], hk) if "dv" in decoders else 0):
        po = mp.slot_passes(do_codes.shape[0], 1, hk, call)
        dout = mp.dv_dout(do_codes, po, dtype)[0]
        zv = torch.zeros(sk, hk, d, dtype=dtype)
        dq, dk, dv = mp.standin_bwd(dout, q, krand, zv, torch.zeros_like(q), lse_ref, used)
        worst("dv", mp.dv_check(dv, exp_dv, po[0]))
        exact += int(mp.exact_zero(dq)) + int(mp.exact_zero(dk))
        if wrong is not None:
            fails += mp.dv_failures(dv, exp_dv, po[0], sq, ratio)
    if first_only and fails:
        return devs, exact, fails
    for code in ((0, 1) if "dq" in decoders else ()):
        a, o0, kc, exp_dq = mp.dq_probe(sq, sk, mask, d, code, dtype, max_k)
        v = torch.zeros(sk, hk, d, dtype=dtype)
        v[:, :, 0] = a.to(dtype)[:, None]
        dout = torch.zeros(sq, h, d, dtype=dtype)
        dout[:, :, 0] = 1
        out = torch.zeros(sq, h, d, dtype=dtype)
        out[:, :, 0] = o0[:, None]
        for call in range(mp.n_calls(kc.shape[0], hk)):
            po = mp.slot_passes(kc.shape[0], 1, hk, call)
            k = mp.dq_keys(kc, po, dtype)[0]
            dq, dk, _ = mp.standin_bwd(dout, q, k, v, out, lse_ref, used)
            poh = po[0].repeat_interleave(ratio)
            dev, ex = mp.dq_check(dq, vis, exp_dq, poh)
            worst("dq", dev)
            exact += int(ex) + int(mp.exact_zero(dk))
            if wrong is not None:
                fails += mp.dq_failures(dq, vis, exp_dq, poh)
    return devs, exact, fails


def fixed_cases():
    return [(sq, sk, m, None) for (sq, sk), m in itertools.product(mp.SHAPES, mp.MASKS)]


def cache_cases():
    return [(sq, sk, m, None) for sq, sk, m in itertools.product(mp.CACHE_SQ, [n for n in mp.CACHE_LENS if n > 0], mp.CACHE_MASKS)]


def packed_cases(lens_k):
    """One case per mask: the batch's non-empty sequences, the window normalised by the longest key sequence of cu_seqlens_k."""
    max_k = max(mp.PACKED_LENS_K)
    return [[(sq, sk, m, max_k) for sq, sk in zip(mp.PACKED_LENS_Q, lens_k) if sq > 0 and sk > 0] for m in mp.MASKS]


def _ratio(case, cache=False):
    """The group ratio of a case, from shape + mask: every mask meets every ratio over the shapes."""
    sq, sk, m = case[0][:3] if isinstance(case, list) else case[:3]
    idx = sq + sk + (mp.CACHE_MASKS if cache else mp.MASKS).index(m)
    return ((4, 8) if cache else (1, 2, 4))[idx % (2 if cache else 3)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_correct_masks_pass_with_room(dtype, d):
    worst = {}
    seqs = [(c, False) for c in fixed_cases()] + [(c, True) for c in cache_cases()] + \
           [(c, False) for lens in (mp.PACKED_LENS_K, mp.PACKED_SEQUSED_K) for batch in packed_cases(lens) for c in batch]
    for idx, ((sq, sk, m, max_k), cache) in enumerate(seqs):
        ratio = _ratio((sq, sk, m), cache)
        devs, exact, _ = run_probe(sq, sk, m, max_k, dtype, d, 2 if idx % 2 else 1, ratio)
        assert exact == 0, (sq, sk, mp.mask_name(m), ratio)
        for nm, x in devs.items():
            assert x <= PASS_BOUND, f"{nm}: deviation {x:.4f} > {PASS_BOUND} at Sq {sq} Sk {sk} mask {mp.mask_name(m)} ratio {ratio}"
            worst[nm] = max(worst.get(nm, 0.0), x)
    print("worst deviations of the stand-in:", {k: round(v, 4) for k, v in sorted(worst.items())})


def _domain(name):
    """[(case = the sequences probed together, from the cache shapes?)]"""
    fixed, cache = [([c], False) for c in fixed_cases()], [([c], True) for c in cache_cases()]
    if name in ("row_mod_sq", "row_div_g"):
        return fixed + cache
    if name == "masked_row_key":
        return [(c, f) for c, f in fixed + cache if c[0][0] > c[0][1]]
    if name == "own_sk":
        return [(batch, False) for batch in packed_cases(mp.PACKED_SEQUSED_K)]
    return fixed


def _hunt(name, case, dtype, d, ratio, decoders=("fwd", "dv", "dq")):
    """Is the mutant different from the right mask in any sequence of the case?  Every such sequence must be reported, in a row that differs."""
    live = False
    for sq, sk, m, max_k in case:
        good = mp.visible(sq, sk, m, max_k)
        wrong = mp.mutant_mask(name, sq, sk, m, max_k, g=ratio)
        if wrong is None or bool((wrong == good).all()):
            continue
        live = True
        differs = (wrong != good).reshape(-1, sq, sk).any(0)
        diff = set(torch.nonzero(differs.any(1)).flatten().tolist())
        if decoders == ("dq",):
            # the dQ decoder's bound is for rows with n_i >= 2.  A row whose ONLY key is lost, or swapped for one other key of the same sign and column class (top-left
            # alignment under window (0, 0) at Sk - Sq = 128), sums a_j - delta_i = 0 either way: nothing to show -- the forward and the dV decoder see it
            n_good, n_wrong = good.sum(1), wrong.reshape(-1, sq, sk).sum(2).max(0).values
            if all(int(n_good[i]) <= 1 and int(n_wrong[i]) <= 1 for i in diff):
                continue
        _, exact, fails = run_probe(sq, sk, m, max_k, dtype, d, 1, ratio, wrong=wrong, first_only=True, decoders=decoders)
        where = f"mutant {name} at Sq {sq} Sk {sk} mask {mp.mask_name(m)} ratio {ratio} d {d} decoders {decoders}"
        assert fails, "the probe did not notice " + where
        for msg, _, rows in fails:
            assert diff & set(rows), f"{where}: reported outside the rows that differ ({sorted(diff)[:6]}..): {msg}"
    return live


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", mp.MUTANTS)
def test_every_mutant_is_caught_in_a_row_that_differs(name, dtype, d):
    domain = _domain(name)
    n_live = sum(_hunt(name, case, dtype, d, _ratio(case, cache)) for case, cache in domain)
    assert 3 * n_live >= len(domain), f"mutant {name} is live in {n_live} of {len(domain)} cases: less than one third"


@pytest.mark.parametrize("decoder", ["dv", "dq"])
@pytest.mark.parametrize("name", ["wr+1", "wr-1", "wl+1", "wl-1", "top_left", "seam_tile", "last_key"])
def test_backward_decoders_report_on_their_own(name, decoder):
    """The forward decoders catch every wrong mask first, so the hunt above never reaches the backward ones: here the dV decoder and the dQ decoder each stand
    alone (the lse handed to the backward is the right mask's, as on the GPU).  bf16 at head dim 64 and fp16 at 128 in turn."""
    n_live = 0
    for idx, (case, _) in enumerate(_domain(name)):
        n_live += _hunt(name, case, DTYPES[idx % 2], (64, 128)[idx % 2], _ratio(case), decoders=(decoder,))
    assert n_live > 0


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_own_sk_is_caught_on_the_plain_packed_batch_too(dtype, d):
    batch = packed_cases(mp.PACKED_LENS_K)[mp.MASKS.index((False, 255, 256))]
    assert _hunt("own_sk", batch, dtype, d, 2)


def test_cap_is_asserted_before_anything_runs():
    vis = mp.visible(64, 1100, (False, -1, -1))
    codes = torch.zeros(1, 1100, 64)
    codes[0, :, 0] = 1.0
    with pytest.raises(AssertionError, match="cap 16"):
        mp.fwd_expected(vis, codes)
