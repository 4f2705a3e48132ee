"""Census of the library's __global__ instantiations (test infrastructure only): one recipe per compiled kernel.

Every instantiation of libfa_gfx950.so is its own compilation -- its own register allocation and, for about 30 of them, its own spills -- and the
dispatch reaches the rare feature products only when a call asks for exactly that product.  This helper holds

  * kernel_metadata(): the kernels of the library's code objects with their resource notes (tests/test_kernel_resources_cpu.py reads the same);
  * parse_symbol(): Itanium-mangled kernel symbol -> key (family, dtype, template ints / bools in order);
  * RECIPES: rows {id, kind, keys, knobs, ...call}: the call, the knobs that pin the dispatch and the keys the call must reach;
  * the checks both census tests share: unclaimed_kernels / stale_keys (table against library, tests/test_kernel_census_cpu.py) and
    missing_from_log (a recipe's keys against the launch log of its call, tests/test_kernel_census_gpu.py).

Shapes (every row): B = 2, H / Hk = 4 / 2 where the path takes grouped heads, two query blocks with the second partial (block rows + 37: 165 rows on the
128-row kernels, 293 on the 256-row ones), at least three key tiles of 64 with the last partial (forward Sk = 203; backward one key block + 75: 331 at head
dims <= 128, 203 above), Sq != Sk, so a causal diagonal is bottom-right aligned off a block edge."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flash-attention_amd", "libfa_gfx950.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernel_metadata():
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in tools):
        pytest.skip("library not built or LLVM binutils not found")
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([tools[0], f"--dump-section=.hip_fatbin={fat}", LIB, os.path.join(tmp, "copy.so")])
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]   # one bundle per translation unit
        for i, p in enumerate(starts):
            piece, obj = os.path.join(tmp, f"b{i}.bin"), os.path.join(tmp, f"co{i}.o")
            open(piece, "wb").write(data[p:starts[i + 1] if i + 1 < len(starts) else len(data)])
            subprocess.check_call([tools[1], "--unbundle", "--type=o", f"--input={piece}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={obj}"])
            notes = subprocess.run([tools[2], "--notes", obj], capture_output=True, text=True, check=True).stdout
            for block in notes.split("- .agpr_count:")[1:]:
                f = {k: v for k, v in re.findall(r"\.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\S+)", block)}
                kernels[f["name"]] = {k: int(v) for k, v in f.items() if k != "name"}
    return kernels


def template_ints(name):
    """Integer template arguments of an Itanium-mangled fa:: kernel name, in order."""
    return [int(x) for x in re.findall(r"Li(\d+)E", name)]


_DTYPES = {"DF16b": "bf16", "DF16_": "f16", "NS_4e4m3E": "e4m3"}
_ARG = re.compile(r"DF16b|DF16_|NS_4e4m3E|Li(\d+)E|Lb([01])E")


def parse_symbol(sym):
    """'_ZN2fa<len><name>[I<args>E]...' -> (family, dtype or None, (ints / bools in order)); None if the symbol is not a kernel of namespace fa in that form."""
    m = re.match(r"_ZN2fa(\d+)", sym)
    if not m:
        return None
    n, at = int(m.group(1)), m.end()
    family, rest = sym[at:at + n], sym[at + n:]
    if len(family) != n or not family.endswith("_kernel"):
        return None
    dtype, args = None, []
    if rest.startswith("I"):   # template arguments: types first (at most one element type), then integers / bools
        pos = 1
        while True:
            a = _ARG.match(rest, pos)
            if not a:
                break
            if a.group(0) in _DTYPES:
                if dtype is not None:
                    return None
                dtype = _DTYPES[a.group(0)]
            elif a.group(1) is not None:
                args.append(int(a.group(1)))
            else:
                args.append(a.group(2) == "1")
            pos = a.end()
        if not rest.startswith("EEv", pos):   # end of the arguments, end of the name, void
            return None
    elif not rest.startswith("E"):
        return None
    return (family, dtype, tuple(args))


def key_str(key):
    family, dtype, args = key
    return "%s<%s>" % (family, ",".join(([dtype] if dtype else []) + [str(a).lower() if isinstance(a, bool) else str(a) for a in args]))


# ---- the checks ----------------------------------------------------------------------------------------------------------------------------
def claimed_keys(recipes):
    return {k for r in recipes for k in r["keys"]}


def unclaimed_kernels(symbols, recipes):
    """Symbols of the library no recipe claims (a symbol that does not parse is unclaimed by definition), by name."""
    claimed = claimed_keys(recipes)
    return sorted(s for s in symbols if parse_symbol(s) not in claimed)


def stale_keys(symbols, recipes):
    """(recipe id, key) pairs whose key no kernel of the library has."""
    have = {parse_symbol(s) for s in symbols}
    return sorted((r["id"], key_str(k)) for r in recipes for k in r["keys"] if k not in have)


def missing_from_log(recipe, log_symbols):
    """Keys the recipe claims that the launch log of its call does not hold: [] = the call reached every code object it claims."""
    got = {parse_symbol(s) for s in log_symbols}
    return [key_str(k) for k in recipe["keys"] if k not in got]


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
NONE, CAP, ALIBI, DROP, ALL, EXACT = 0, 1, 2, 4, 7, 8   # csrc/fa_device.h FEAT_*
DTS = ("bf16", "f16")
MODES = ("full", "causal")
WINDOW = (70, 30)   # the two-sided window of the one "local" row per family
# feature code -> (softcap, alibi, dropout) of the call; FEAT_ALL is the run-time-checked variant: softcap + ALiBi, under a causal mask with dropout too
_FEATS = {NONE: (0.0, False, 0.0), CAP: (30.0, False, 0.0), ALIBI: (0.0, True, 0.0), DROP: (0.0, False, 0.1), CAP | DROP: (5.0, False, 0.25),
          ALIBI | DROP: (0.0, True, 0.1), ALL: (30.0, True, 0.0)}
_FNAME = {NONE: "plain", CAP: "cap", ALIBI: "alibi", DROP: "drop", CAP | DROP: "cap+drop", ALIBI | DROP: "alibi+drop", ALL: "all"}
SEVEN = (NONE, CAP, ALIBI, DROP, CAP | DROP, ALIBI | DROP, ALL)
PAIR_OFF = {"FA_BWD_MODE": 1, "FA_BWD_GSPLIT": 0}   # backward rows: the recomputing pair on unsplit GQA groups (the fused / chunked launches and the group split have rows of their own)

RECIPES = []


def K(family, dtype, *args):
    return (family, dtype, tuple(args))


def _row(id_, kind, keys, knobs=None, **call):
    RECIPES.append(dict(id=id_, kind=kind, keys=list(keys), knobs=dict(knobs or {}), **call))


def _attn(id_, keys, knobs, dt, d, sq, sk, mode, feat=NONE, varlen=False, replay=False):
    """fa_fwd / fa_varlen_fwd and their backward through the public functions (tools/fuzz_gpu.py run_case)."""
    cap, alibi, pd = _FEATS[feat]
    if feat == ALL and mode == "causal":
        pd = 0.1
    _row(id_, "attn", keys, knobs, dt=dt, d=d, sq=sq, sk=sk, mode=mode, window=WINDOW if mode == "local" else (-1, -1), cap=cap, alibi=alibi, pd=pd,
         varlen=varlen, replay=replay)


def _dkdv_feat(feat, prescale=False):
    return feat if feat != NONE else (NONE if prescale else EXACT)


def _build():
    for dt in DTS:
        # -- lock-step forward, head dims 64 / 128: <E, D, DV, NW, FEAT, PP>, 4 / 8 waves x seven feature variants, 8-wave ping-pong plain / all-features
        for d in (64, 128):
            for mode in MODES + (("local",) if (dt, d) == ("bf16", 128) else ()):
                for nw in (4, 8):
                    for f in SEVEN if mode != "local" else (NONE,):
                        if mode == "local" and nw == 8:
                            continue
                        _attn(f"fwd-{dt}-d{d}-nw{nw}-{_FNAME[f]}-{mode}", [K("fa_fwd_kernel", dt, d, d, nw, f, False)], {"FA_FWD_NW": nw}, dt, d, 32 * nw + 37, 203, mode, f)
                if mode == "local":
                    continue
                for f in (NONE, ALL):
                    _attn(f"fwd-{dt}-d{d}-pingpong-{_FNAME[f]}-{mode}", [K("fa_fwd_kernel", dt, d, d, 8, f, True)], {"FA_FWD_NW": 16}, dt, d, 293, 203, mode, f)
                # -- pipelined forward: <E, D, NW, SCHED>
                for nw in (4, 8):
                    for sched in (0, 3):
                        _attn(f"fwd_il-{dt}-d{d}-nw{nw}-sched{sched}-{mode}", [K("fa_fwd_il_kernel", dt, d, nw, sched)], {"FA_FWD_NW": 30 + nw, "FA_IL_SCHED": sched},
                              dt, d, 32 * nw + 37, 203, mode)
                # -- 64-rows-per-wave forward: <E, D, FEAT, PAGED, DENSE>; dense = a fixed-length batch without a left window, else (packed batch, window) the general one
                w64 = {"FA_FWD_NW": 64}
                _attn(f"fwd_w64-{dt}-d{d}-dense-{mode}", [K("fa_fwd_w64_kernel", dt, d, NONE, False, True)], w64, dt, d, 293, 203, mode)
                _attn(f"fwd_w64-{dt}-d{d}-varlen-{mode}", [K("fa_fwd_w64_kernel", dt, d, NONE, False, False)], w64, dt, d, 293, 203, mode, varlen=True)
                _attn(f"fwd_w64-{dt}-d{d}-cap-{mode}", [K("fa_fwd_w64_kernel", dt, d, CAP, False, False)], w64, dt, d, 293, 203, mode, CAP)
                _attn(f"fwd_w64-{dt}-d{d}-drop-{mode}", [K("fa_fwd_w64_kernel", dt, d, DROP, False, False)], w64, dt, d, 293, 203, mode, DROP, replay=True)
                if mode == "causal":   # the bias rides in the score chains only where no visible key lies right of the diagonal
                    _attn(f"fwd_w64-{dt}-d{d}-alibi-{mode}", [K("fa_fwd_w64_kernel", dt, d, ALIBI, False, False)], w64, dt, d, 293, 203, mode, ALIBI)
                _row(f"fwd_w64-{dt}-d{d}-paged-{mode}", "kvcache", [K("fa_fwd_w64_kernel", dt, d, NONE, True, False)], w64, dt=dt, d=d, sq=293, cap=512, lens=(331, 459),
                     paged=True, causal=mode == "causal", window=(-1, -1), splits=0)
        _attn(f"fwd_il-{dt}-d128-nw4-sched3-local", [K("fa_fwd_il_kernel", dt, 128, 4, 3)], {"FA_FWD_NW": 34}, dt, 128, 165, 203, "local")
        _attn(f"fwd_w64-{dt}-d128-general-local", [K("fa_fwd_w64_kernel", dt, 128, NONE, False, False)], {"FA_FWD_NW": 64}, dt, 128, 293, 203, "local")

        # -- backward pair, head dims 64 / 128: delta <E, D, DV, DVV>, dQ <E, D, DV, NW, FEAT, DVV> (4 / 8 waves), dK/dV <E, D, DV, FEAT, DVV> (plain = FEAT_EXACT,
        # or FEAT_NONE under FA_DKDV_PRESCALE: the 8-wave dQ rows carry that knob)
        for d in (64, 128):
            for mode in MODES + (("local",) if (dt, d) == ("bf16", 128) else ()):
                for nw in (4, 8):
                    for f in SEVEN if mode != "local" else (NONE,):
                        if mode == "local" and nw == 8:
                            continue
                        pre = nw == 8
                        _attn(f"bwd-{dt}-d{d}-dq{nw}-{_FNAME[f]}-{mode}",
                              [K("fa_bwd_delta_kernel", dt, d, d, d), K("fa_bwd_dq_kernel", dt, d, d, nw, f, d), K("fa_bwd_dkdv_kernel", dt, d, d, _dkdv_feat(f, pre), d)],
                              dict(PAIR_OFF, FA_BWD_DQ_NW=nw, FA_BWD_DKDV=8, FA_DKDV_PRESCALE=int(pre)), dt, d, 32 * nw + 37, 331, mode, f)
        # -- 64-per-wave backward kernels: dQ <E, D, FUSE_DELTA, FEAT> (softcap / dropout: head dim 128, fused delta only), dK/dV <E, D, FEAT> (plain, causal ALiBi, softcap at 128)
        for d in (64, 128):
            for fuse in (1, 0):
                kn = dict(PAIR_OFF, FA_BWD_DQ_NW=64, FA_BWD_DKDV=64, FA_BWD_FUSE_DELTA=fuse)
                delta = [] if fuse else [K("fa_bwd_delta_kernel", dt, d, d, d)]
                for mode in MODES + (("local",) if (dt, d, fuse) == ("bf16", 128, 1) else ()):
                    _attn(f"bwd_w64-{dt}-d{d}-fuse{fuse}-plain-{mode}", delta + [K("fa_bwd_dq_w64_kernel", dt, d, bool(fuse), NONE), K("fa_bwd_dkdv_w64_kernel", dt, d, NONE)], kn,
                          dt, d, 293, 331, mode)
                _attn(f"bwd_w64-{dt}-d{d}-fuse{fuse}-alibi-causal", delta + [K("fa_bwd_dq_w64_kernel", dt, d, bool(fuse), ALIBI), K("fa_bwd_dkdv_w64_kernel", dt, d, ALIBI)], kn,
                      dt, d, 293, 331, "causal", ALIBI)
            if d == 128:
                kn = dict(PAIR_OFF, FA_BWD_DQ_NW=64, FA_BWD_DKDV=64)
                for mode in MODES:
                    _attn(f"bwd_w64-{dt}-d128-fuse1-cap-{mode}", [K("fa_bwd_dq_w64_kernel", dt, 128, True, CAP), K("fa_bwd_dkdv_w64_kernel", dt, 128, CAP)], kn, dt, 128, 293, 331, mode, CAP)
                    # (dropout: the dQ kernel only; dK/dV stays on the eight-wave kernel)
                    _attn(f"bwd_w64-{dt}-d128-fuse1-drop-{mode}", [K("fa_bwd_dq_w64_kernel", dt, 128, True, DROP), K("fa_bwd_dkdv_kernel", dt, 128, 128, DROP, 128)], kn, dt, 128, 293, 331, mode, DROP)
            # -- the fused launch and the 5-contraction launches: plain attention, fixed length, sk >= sq, no left window (so no window row)
            for mode in MODES:
                _attn(f"bwd_fused-{dt}-d{d}-{mode}", [K("fa_bwd_delta_kernel", dt, d, d, d), K("fa_bwd_fused_kernel", dt, d)], {"FA_BWD_MODE": 3, "FA_BWD_GSPLIT": 0}, dt, d, 293, 331, mode)
                _attn(f"bwd_c5-{dt}-d{d}-{mode}", [K("fa_bwd_delta_kernel", dt, d, d, d), K("fa_bwd_c5_kernel", dt, d)], {"FA_BWD_MODE": 5, "FA_BWD_GSPLIT": 0}, dt, d, 293, 331, mode)
        # -- the sum of a split GQA group's partial dK / dV
        for mode in MODES:
            _attn(f"bwd_gsum-{dt}-{mode}", [K("fa_bwd_gsum_kernel", dt)], {"FA_BWD_MODE": 1, "FA_BWD_GSPLIT": 2, "FA_BWD_DQ_NW": 4, "FA_BWD_DKDV": 8}, dt, 128, 165, 331, mode)

        # -- head dim 256 (4 waves; forward and backward share the call: both sides want Sk = 203) and the trimmed head dims 32 / 96 / 192 (plain and all-features only)
        for mode in MODES:
            for f in SEVEN:
                _attn(f"d256-{dt}-{_FNAME[f]}-{mode}",
                      [K("fa_fwd_kernel", dt, 256, 256, 4, f, False), K("fa_bwd_delta_kernel", dt, 256, 256, 256), K("fa_bwd_dq_kernel", dt, 256, 256, 4, f, 256),
                       K("fa_bwd_dkdv_kernel", dt, 256, 256, _dkdv_feat(f), 256)], PAIR_OFF, dt, 256, 165, 203, mode, f)
            _attn(f"d256-{dt}-prescale-{mode}", [K("fa_bwd_dkdv_kernel", dt, 256, 256, NONE, 256)], dict(PAIR_OFF, FA_DKDV_PRESCALE=1), dt, 256, 165, 203, mode)
            for f in (NONE, ALL):
                _attn(f"d192-{dt}-{_FNAME[f]}-{mode}",
                      [K("fa_fwd_kernel", dt, 256, 192, 4, f, False), K("fa_bwd_delta_kernel", dt, 256, 192, 192), K("fa_bwd_dq_kernel", dt, 256, 192, 4, f, 192),
                       K("fa_bwd_dkdv_kernel", dt, 256, 192, _dkdv_feat(f), 192)], PAIR_OFF, dt, 192, 165, 203, mode, f)
            _attn(f"d192-{dt}-prescale-{mode}", [K("fa_bwd_dkdv_kernel", dt, 256, 192, NONE, 192)], dict(PAIR_OFF, FA_DKDV_PRESCALE=1), dt, 192, 165, 203, mode)
            for dv, d in ((32, 64), (96, 128)):
                for f in (NONE, ALL):
                    _attn(f"d{dv}-{dt}-fwd-{_FNAME[f]}-{mode}", [K("fa_fwd_kernel", dt, d, dv, 4, f, False)], {}, dt, dv, 165, 203, mode, f)
                    _attn(f"d{dv}-{dt}-bwd-{_FNAME[f]}-{mode}",
                          [K("fa_bwd_delta_kernel", dt, d, dv, dv), K("fa_bwd_dq_kernel", dt, d, dv, 4, f, dv), K("fa_bwd_dkdv_kernel", dt, d, dv, _dkdv_feat(f), dv)], PAIR_OFF,
                          dt, dv, 165, 331, mode, f)
                _attn(f"d{dv}-{dt}-bwd-prescale-{mode}", [K("fa_bwd_dkdv_kernel", dt, d, dv, NONE, dv)], dict(PAIR_OFF, FA_DKDV_PRESCALE=1), dt, dv, 165, 331, mode)

        # -- q / k head dim 192 with v / o head dim 128: forward <E, 192, 128, 4> and the 256-pitch backward kernels with a value width of their own
        for mode in MODES + ("local",):
            _row(f"dv192_128-{dt}-{mode}", "dv",
                 [K("fa_fwd_dv_kernel", dt, 192, 128, 4), K("fa_bwd_delta_kernel", dt, 256, 192, 128), K("fa_bwd_dq_kernel", dt, 256, 192, 4, NONE, 128),
                  K("fa_bwd_dkdv_kernel", dt, 256, 192, EXACT, 128)], PAIR_OFF, dt=dt, sq=165, sk=203, mode=mode)

        # -- split keys: one query row, Sk = 700, three splits; the 4-wave lock-step kernel writes partials, the combine <E, D, DV> merges them (a single row has no causal mask)
        for dv, d in ((32, 64), (64, 64), (96, 128), (128, 128), (192, 256), (256, 256)):
            _row(f"split-{dt}-d{dv}", "kvcache", [K("fa_fwd_kernel", dt, d, dv, 4, NONE, False), K("fa_splitkv_combine_kernel", dt, d, dv)], {}, dt=dt, d=dv, sq=1, cap=700, lens=(700, 389),
                 paged=False, causal=False, window=(-1, -1), splits=3)
        _row(f"split-{dt}-d128-paged", "kvcache", [K("fa_fwd_kernel", dt, 128, 128, 4, NONE, False), K("fa_splitkv_combine_kernel", dt, 128, 128)], {}, dt=dt, d=128, sq=1, cap=768,
             lens=(700, 389), paged=True, causal=False, window=(-1, -1), splits=3)
        # -- absorbed MLA decode <E, 576, 512, 4>: 64 packed rows per block (51 rows x 2 heads of a group = two blocks, the second partial), and its split form
        for mode in MODES + ("local",):
            _row(f"mla-{dt}-{mode}", "mla", [K("fa_fwd_mla_kernel", dt, 576, 512, 4)], {}, dt=dt, sq=51, cap=203, lens=(203, 150), layout="contig", mode=mode, splits=1)
        _row(f"mla-{dt}-paged-causal", "mla", [K("fa_fwd_mla_kernel", dt, 576, 512, 4)], {}, dt=dt, sq=51, cap=512, lens=(331, 459), layout="paged256", mode="causal", splits=1)
        _row(f"mla-{dt}-split", "mla", [K("fa_fwd_mla_kernel", dt, 576, 512, 4), K("fa_splitkv_combine_kernel", dt, 512, 512)], {}, dt=dt, sq=1, cap=700, lens=(700, 389), layout="contig",
             mode="full", splits=3)
        _row(f"rotary-{dt}", "rotary", [K("fa_rotary_kernel", dt)], {}, dt=dt)

    # -- FP8 forwards: <D> and, against an fp8 KV cache, <e4m3, D, RING> (FA_FP8_KV_RING staging slots)
    for d in (64, 128):
        for mode in MODES + (("local",) if d == 128 else ()):
            _row(f"fp8-d{d}-{mode}", "fp8", [K("fa_fwd_fp8_kernel", None, d)], {}, d=d, sq=165, sk=203, mode=mode)
            for ring in (2, 3, 4):
                if mode == "local" and ring != 4:
                    continue
                _row(f"fp8kv-d{d}-ring{ring}-{mode}", "fp8kv", [K("fa_fwd_fp8_kv_kernel", "e4m3", d, ring)], {"FA_FP8_KV_RING": ring}, d=d, sq=165, cap=256, lens=(203, 150), layout="contig",
                     mode=mode, splits=1)
        _row(f"fp8kv-d{d}-ring4-paged-causal", "fp8kv", [K("fa_fwd_fp8_kv_kernel", "e4m3", d, 4)], {"FA_FP8_KV_RING": 4}, d=d, sq=165, cap=512, lens=(331, 459), layout="paged256",
             mode="causal", splits=1)
    # -- the three untemplated kernels
    _row("kv_append", "append", [K("fa_kv_append_kernel", None)], {})
    _row("varlen_schedule", "schedule", [K("fa_varlen_schedule_kernel", None)], {"FA_FWD_NW": 4})
    _row("set_rng", "set_rng", [K("fa_set_rng_kernel", None)], {})


_build()
assert len({r["id"] for r in RECIPES}) == len(RECIPES), "recipe ids are unique"
