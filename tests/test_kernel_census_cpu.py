"""The census table against the built library, no GPU (tests/_kernel_census.py): every __global__ instantiation in the library's code objects is claimed by a
recipe and every key a recipe claims is a kernel of the library -- symbol for symbol, both directions, no exclusions.  A new instantiation without a recipe
fails here; an instantiation no call can reach is dead code and leaves the build instead of entering a list.  The negative controls run the same check
functions on fabricated inputs, the launch-log check of tests/test_kernel_census_gpu.py among them."""
import pytest

from tests import _kernel_census as kc


@pytest.fixture(scope="module")
def symbols():
    return sorted(kc.kernel_metadata())


def test_parser_reads_every_form():
    assert kc.parse_symbol("_ZN2fa13fa_fwd_kernelIDF16bLi128ELi96ELi4ELi7ELb0EEEvNS_4FwdKE") == ("fa_fwd_kernel", "bf16", (128, 96, 4, 7, False))
    assert kc.parse_symbol("_ZN2fa17fa_fwd_w64_kernelIDF16_Li64ELi0ELb1ELb0EEEvNS_4FwdKE") == ("fa_fwd_w64_kernel", "f16", (64, 0, True, False))
    assert kc.parse_symbol("_ZN2fa20fa_fwd_fp8_kv_kernelINS_4e4m3ELi128ELi3EEEvNS_4FwdKENS_4Fp8KE") == ("fa_fwd_fp8_kv_kernel", "e4m3", (128, 3))
    assert kc.parse_symbol("_ZN2fa17fa_fwd_fp8_kernelILi64EEEvNS_4FwdKENS_4Fp8KE") == ("fa_fwd_fp8_kernel", None, (64,))
    assert kc.parse_symbol("_ZN2fa18fa_bwd_gsum_kernelIDF16bEEvPKT_PS1_xiiiilll") == ("fa_bwd_gsum_kernel", "bf16", ())
    assert kc.parse_symbol("_ZN2fa17fa_set_rng_kernelEmmPm") == ("fa_set_rng_kernel", None, ())
    for bad in ("fa_fwd_kernel", "_ZN2fa13launch_rotaryERKNS_7RotaryKEiP12ihipStream_t", "_ZN2fa13fa_fwd_kernelIfLi128EEEvNS_4FwdKE", "?"):
        assert kc.parse_symbol(bad) is None, bad
    assert kc.template_ints("_ZN2fa13fa_fwd_kernelIDF16bLi128ELi96ELi4ELi7ELb0EEEvNS_4FwdKE") == [128, 96, 4, 7]


def test_every_kernel_of_the_library_has_a_recipe(symbols):
    assert len(symbols) >= 250, len(symbols)
    assert all(kc.parse_symbol(s) is not None for s in symbols), [s for s in symbols if kc.parse_symbol(s) is None]
    assert len({kc.parse_symbol(s) for s in symbols}) == len(symbols)   # the key keeps every template argument: no two kernels share one
    assert kc.unclaimed_kernels(symbols, kc.RECIPES) == []


def test_every_claimed_key_is_a_kernel_of_the_library(symbols):
    assert kc.stale_keys(symbols, kc.RECIPES) == []


def test_rows_are_well_formed():
    kinds = {"attn", "kvcache", "mla", "dv", "fp8", "fp8kv", "rotary", "append", "schedule", "set_rng"}
    for r in kc.RECIPES:
        assert r["kind"] in kinds and r["keys"], r["id"]
        assert all(k.startswith("FA_") for k in r["knobs"]), r["id"]
        assert "FA_DEBUG_LAUNCH_LOG" not in r["knobs"]   # the GPU test sets it for every row


def test_negative_controls():
    symbols = ["_ZN2fa16fa_rotary_kernelIDF16bEEvNS_7RotaryKE", "_ZN2fa17fa_set_rng_kernelEmmPm"]
    rows = [dict(id="rotary-bf16", kind="rotary", keys=[kc.K("fa_rotary_kernel", "bf16")], knobs={}),
            dict(id="set_rng", kind="set_rng", keys=[kc.K("fa_set_rng_kernel", None)], knobs={})]
    assert kc.unclaimed_kernels(symbols, rows) == [] and kc.stale_keys(symbols, rows) == []
    # an extra symbol in the library is reported by name (one that parses and one that does not)
    extra = "_ZN2fa16fa_rotary_kernelIDF16_EEvNS_7RotaryKE"
    assert kc.unclaimed_kernels(symbols + [extra], rows) == [extra]
    assert kc.unclaimed_kernels(symbols + ["_ZN2fa9fa_weirdoIfEEvv"], rows) == ["_ZN2fa9fa_weirdoIfEEvv"]
    # a recipe whose key no kernel has is reported with its id
    stale = dict(id="rotary-f16", kind="rotary", keys=[kc.K("fa_rotary_kernel", "f16")], knobs={})
    assert kc.stale_keys(symbols, rows + [stale]) == [("rotary-f16", "fa_rotary_kernel<f16>")]
    # the launch-log check: a log without the claimed key fails, a sibling instantiation does not count, the exact kernel passes
    row = dict(id="x", kind="attn", keys=[kc.K("fa_fwd_kernel", "bf16", 128, 128, 4, 0, False), kc.K("fa_bwd_delta_kernel", "bf16", 128, 128, 128)], knobs={})
    exact = ["_ZN2fa13fa_fwd_kernelIDF16bLi128ELi128ELi4ELi0ELb0EEEvNS_4FwdKE", "_ZN2fa19fa_bwd_delta_kernelIDF16bLi128ELi128ELi128EEEvNS_4BwdKE"]
    assert kc.missing_from_log(row, exact) == []
    assert kc.missing_from_log(row, []) == ["fa_fwd_kernel<bf16,128,128,4,0,false>", "fa_bwd_delta_kernel<bf16,128,128,128>"]
    sibling = ["_ZN2fa13fa_fwd_kernelIDF16bLi128ELi128ELi8ELi0ELb0EEEvNS_4FwdKE", exact[1], "?"]
    assert kc.missing_from_log(row, sibling) == ["fa_fwd_kernel<bf16,128,128,4,0,false>"]
