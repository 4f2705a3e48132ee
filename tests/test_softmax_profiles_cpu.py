"""Can the score profiles of tests/_softmax_profiles.py fail?  A torch stand-in of the deferred, lagged online softmax (sp.standin) runs over every case list of
tests/test_softmax_profiles_gpu.py and is judged by the rule the GPU module applies to that list:

  - the faithful stand-in is under every bound, and the builder's conditions hold on every profile (asserted while it is built: sp.check_conditions);
  - each of the nine mutants -- O never scaled, O scaled twice, l not scaled, the pending factor dropped at the epilogue, a pending factor overwritten by a growth in the
    next step, one lane's factor applied to its 32-row group, the growing step's mask lost, the threshold compared with the previous tile's maximum, a first key that does
    not count as growth -- is reported on at least one case of every list where it is live (sp.live: from the plan alone).

With FA_SOFTMAX_PROFILES_REPORT=<file> the stand-in's deviations and every mutant's ratio to its bound on every live case are appended there
(profiles/softmax_profiles.txt holds such a run); without it a list stops at the first case that reports a mutant."""
import os

import pytest
import torch

from tests import _softmax_profiles as sp

LISTS = sp.case_lists()
REPORT = os.environ.get("FA_SOFTMAX_PROFILES_REPORT")


def run(name, spec, mutant=None):
    p, o, l, err_pt = sp.reference(spec)
    out, lse = sp.standin(p, p.thr, mutant)
    return p, sp.judge(out, lse, o, l, sp.out_tolerance(sp.family_of(name), p, o, err_pt), None if p.dtype == "e4m3" else sp.LSE_BOUND)


def _note(line):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("name", list(LISTS))
def test_faithful_standin_is_under_every_bound(name):
    worst_o = worst_l = 0.0
    for spec in LISTS[name]:
        p, (r_o, r_l, problems) = run(name, spec)
        assert not problems, (name, p.mask, p.sq, p.sk, problems)
        worst_o, worst_l = max(worst_o, r_o), max(worst_l, r_l if p.dtype == "e4m3" else r_l * sp.LSE_BOUND)
    _note("standin  %-28s cases %d  out error / bound %.3f  lse %s %.2e" % (name, len(LISTS[name]), worst_o, "rel/5e-4" if "fp8" in name else "abs", worst_l))
    if "fp8" not in name:
        assert 2 * worst_l <= sp.LSE_BOUND, "LSE_BOUND is 2 x the stand-in's worst deviation, never below 2e-3"


@pytest.mark.parametrize("mutant", sp.MUTANTS)
@pytest.mark.parametrize("name", list(LISTS))
def test_every_mutant_is_reported_where_it_is_live(name, mutant):
    ratios = []
    for spec in LISTS[name]:
        if not sp.live(mutant, sp.profile_of(spec)):
            continue
        p, (r_o, r_l, problems) = run(name, spec, mutant)
        ratios.append(max(r_o, r_l) if problems else 0.0)
        if problems and not REPORT:
            break
    if not ratios:
        return   # (not live on this list: nothing was placed for it)
    _note("mutant   %-28s %-14s live on %d, best ratio to the bound %s" % (name, mutant, len(ratios), "%.1f" % max(ratios)))
    assert max(ratios) > 1.0, (name, mutant, "not reported on any of its %d live cases" % len(ratios))


def test_every_mutant_is_live_somewhere_and_lists_hold_their_placements():
    """Nothing was placed in vain: every mutant is live on some list of every forward family it applies to, and every family has at least three distinct placements."""
    profs = {name: [sp.profile_of(s) for s in specs] for name, specs in LISTS.items()}
    for mutant in sp.MUTANTS:
        names = [n for n, ps in profs.items() if any(sp.live(mutant, p) for p in ps)]
        assert names, mutant
        if mutant in ("o_never", "o_twice", "l_not", "epilogue_drop", "overwrite", "first_no_grow"):
            for fam in ("fwd ", "lockstep", "w64 alibi", "w64 softcap", "dv ", "mla ", "kvcache ", "fp8 d", "fp8 kvcache"):
                assert any(n.startswith(fam) for n in names), (mutant, fam)
    for name, ps in profs.items():
        places = set().union(*(sp.placements_of(p.plan) for p in ps))
        assert len(places) >= 3, (name, places)
        if any(p.mask != (False, -1, -1) and p.sq >= 64 for p in ps):
            assert any("+decoy" in x for x in places), (name, places)


def test_rows_without_a_target_see_the_background_alone():
    """The channels of the targets are zero in every other row: without the targets the other rows' scores are the same, bit for bit, in fp32 as well."""
    spec = LISTS["fwd bf16 d64 thr8"][1]
    with_t, without = sp.profile_of(spec), sp.profile_of(spec, targets=False)
    rows = sorted({(t[1], t[2]) for t in with_t.targets})
    keep = torch.ones(with_t.sq, with_t.h, dtype=torch.bool)
    for r, h in rows:
        keep[r, h] = False
    s_a = torch.einsum("ihd,jhd->ihj", with_t.q, with_t.k.repeat_interleave(2, 1))
    s_b = torch.einsum("ihd,jhd->ihj", without.q, without.k.repeat_interleave(2, 1))
    assert torch.equal(s_a[keep], s_b[keep]) and torch.equal(with_t.v, without.v) and not torch.equal(s_a[~keep], s_b[~keep])


def test_the_builder_refuses_what_breaks_its_conditions():
    """check_conditions is an assertion on the finished tensors, not a comment: a fire with too few keys ahead, a visible decoy and a height above the cap are refused."""
    with pytest.raises(AssertionError):   # 100 keys ahead of a default-threshold fire: the keys before it hold ~5 % of the row
        sp.check_conditions(sp.build("bf16", 64, 64, 64, 400, 1, 1, (False, -1, -1), 8, [("fire", 5, 0, [100], None)]))
    with pytest.raises(AssertionError, match="decoy"):
        sp.check_conditions(sp.build("bf16", 64, 64, 64, 400, 1, 1, (False, -1, -1), 0, [("fire", 5, 0, [100], 101)]))
    with pytest.raises(AssertionError, match="cap"):
        sp.build("bf16", 64, 64, 64, 400, 1, 1, (False, -1, -1), 8, [("stairs", 5, 0, [100, 132, 164, 196], None)], softcap=10.0)


def test_softcap_30_would_miss_the_lse_bound_in_bf16():
    """Why the capped profiles use sp.SOFTCAP = 24: the capped kernels fold 0.375 / softcap into the once-rounded Q'.  At 30 that is not a bf16 number, a spike's raw
    score carries 2^-9 of itself into LSE and the stand-in misses LSE_BOUND; at 24 (2^-6) it is exact."""
    spec = LISTS["w64 softcap bf16"][0]
    worse = sp.spec(**dict(dict(spec), softcap=30.0))
    (p, o, l, _), (p30, o30, l30, _) = sp.reference(spec), sp.reference(worse)
    dev = lambda pp, ll: float((sp.standin(pp, 8)[1].double() - ll).abs().max())
    assert dev(p, l) < sp.LSE_BOUND / 2 and dev(p30, l30) > sp.LSE_BOUND
