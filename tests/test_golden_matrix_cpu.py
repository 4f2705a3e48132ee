"""CPU suite: the wider reference-generated matrix (tests/golden/ref_matrix_*.npz, written by tests/golden/make_golden.py from the reference's attention_ref + autograd).
  * the numpy fp64 oracle reproduces out, LSE, dq, dk, dv of every case -- packed batches per sequence on the unpadded slices, zeros at padded rows and keys --
    at the tolerance tests/test_oracle_cpu.py uses for the first 13 cases: this extends the oracle's pinning to padding, odd head dims, group ratios 4 / 6 / 8
    and 2k rows;
  * the bound of tests/test_golden_matrix_gpu.py is one the reference itself meets: its fp32 result rounded to bf16 / fp16 lies inside it for every case and tensor;
  * schema and sizes of the files."""
import os

import numpy as np
import pytest
import torch

from oracle import attention_oracle as orc
from tests._util import MATRIX_FAMILIES, bf16_bits_to_f32, load_matrix, matrix_bound, matrix_files, matrix_meta, matrix_names

CASES = [(f, n) for f in MATRIX_FAMILIES for n in matrix_names(f)]
KEYS = {"q_bf16bits", "k_bf16bits", "v_bf16bits", "do_bf16bits", "out", "dq", "dk", "dv", "lse", "meta", "softcap", "err_pt_bf16", "err_pt_fp16"}
OPTIONAL = {"rows", "qmask", "kmask", "alibi_slopes", "bwd_from_oracle"}
# err_pt entries that are not finite by construction: the reference's softcap branch applies tanh in place, so neither its fp32 nor its bf16 / fp16 form has
# gradients (the fixture's gradients for these two are the oracle's, bwd_from_oracle = 1)
NO_GRAD_YARDSTICK = {"softcap_gqa4_causal_113x203_d32", "softcap_gqa4_full_128x217_d32"}
LARGEST_OLD_FILE, TOTAL_CAP = 6_200_564, 18_000_000   # tests/golden/attention_ref_cases.npz; the matrix as a whole


def _inputs(case):
    return [bf16_bits_to_f32(case[n + "_bf16bits"]).astype(np.float64) for n in ("q", "k", "v", "do")]


def test_matrix_covers_what_it_is_for():
    metas = {n: matrix_meta(load_matrix(f)[n]) for f, n in CASES}
    assert len(metas) >= 35
    assert {40, 59, 111, 160, 192, 224, 32, 64, 128} <= {m["D"] for m in metas.values()}
    assert {1, 2, 3, 4, 6, 8} <= {m["ratio"] for m in metas.values() if not m["packed"]}
    assert sum(m["packed"] for m in metas.values()) >= 8
    pairs = {(m["Sq"], m["Sk"]) for m in metas.values()}
    assert {(113, 203), (128, 217), (113, 211), (108, 256), (256, 512), (512, 256), (1024, 1024), (1023, 1024), (1024, 1023), (2048, 2048), (1, 147)} <= pairs
    # the group split where its indices are not trivially zero: more than one query row, and two kv heads and / or two batch entries
    hard = [m for m in metas.values() if not m["packed"] and m["Sq"] > 1 and m["D"] % 8 == 0]
    mode = lambda m: "causal" if m["causal"] else "local" if m["window"] != (-1, -1) else "full"
    assert {"causal", "local"} <= {mode(m) for m in hard if m["ratio"] == 4 and m["Hk"] == 2 and m["B"] == 2}
    assert {"causal", "local"} <= {mode(m) for m in hard if m["ratio"] == 8} and any(m["ratio"] == 8 and m["B"] == 2 for m in hard)
    assert any(m["ratio"] == 4 and m["Hk"] == 2 and m["Sk"] > 512 for m in hard) and any(m["ratio"] == 3 and m["Hk"] == 2 for m in hard)
    blocks = {-(-m["Sk"] // (128 if m["D"] > 128 else 256)) for m in metas.values() if m["ratio"] in (4, 6, 8) and not m["packed"]}
    assert {1, 2, 3} <= blocks and {4, 8} <= {-(-m["Sk"] // 256) for m in metas.values()}   # key blocks of the dK/dV kernels (fa_bwd.hip bwd_block_n)


@pytest.mark.parametrize("family,name", CASES, ids=[n for _, n in CASES])
def test_schema(family, name):
    case = load_matrix(family)[name]
    assert KEYS <= set(case) <= KEYS | OPTIONAL, sorted(set(case) ^ KEYS)
    m = matrix_meta(case)
    B, Sq, Sk, H, Hk, D = (m[x] for x in ("B", "Sq", "Sk", "H", "Hk", "D"))
    assert H % Hk == 0 and case["q_bf16bits"].shape == case["do_bf16bits"].shape == (B, Sq, H, D) and case["k_bf16bits"].shape == case["v_bf16bits"].shape == (B, Sk, Hk, D)
    assert all(case[x + "_bf16bits"].dtype == np.uint16 for x in "qkv") and all(case[x].dtype == np.float32 for x in ("out", "dq", "dk", "dv", "lse"))
    for x in _inputs(case):   # exact in bf16 by storage; exact in fp16 too: nothing below its smallest normal, nothing above its largest
        assert np.all((x == 0) | (np.abs(x) >= 2.0 ** -14)) and np.abs(x).max() < 65504 and np.array_equal(x.astype(np.float16).astype(np.float64), x)
    nrows = Sq
    if (Sq >= 1024) != ("rows" in case):
        pytest.fail("row sample exactly where Sq >= 1024")
    if "rows" in case:
        rows = case["rows"]
        nrows = len(rows)
        assert rows.dtype == np.int64 and np.all(np.diff(rows) > 0) and rows[0] == 0 and rows[-1] == Sq - 1
        assert set(range(128)) | set(range(Sq - 128, Sq)) | set(range(0, Sq, 16)) == set(rows.tolist())
    assert case["out"].shape == case["dq"].shape == (B, nrows, H, D) and case["lse"].shape == (B, H, nrows) and case["dk"].shape == case["dv"].shape == (B, Sk, Hk, D)
    assert m["packed"] == ("kmask" in case)
    if m["packed"]:
        assert case["qmask"].shape == (B, Sq) and case["kmask"].shape == (B, Sk) and case["qmask"].dtype == np.bool_
        for mask in (case["qmask"], case["kmask"]):   # lengths: ones first
            assert all(np.array_equal(r, np.arange(len(r)) < r.sum()) for r in mask)
    if m["window"] != (-1, -1):
        assert not m["causal"] and min(m["window"]) >= 0   # explicit bounds on both sides
    if m["alibi"] is not None:
        assert m["alibi"].shape == (B, H) and m["alibi"].dtype == np.float32
    assert m["bwd_from_oracle"] == (m["softcap"] > 0) == (name in NO_GRAD_YARDSTICK)
    for key in ("err_pt_bf16", "err_pt_fp16"):
        e = case[key]
        assert e.shape == (4,) and np.isfinite(e[0]) and e[0] > 0
        assert np.all(np.isnan(e[1:])) if name in NO_GRAD_YARDSTICK else (np.all(np.isfinite(e)) and np.all(e > 0)), (key, e)
    assert np.all(case["err_pt_fp16"][:1] < case["err_pt_bf16"][:1])


def test_file_sizes():
    sizes = [os.path.getsize(p) for f in MATRIX_FAMILIES for p in matrix_files(f)]
    assert sizes and max(sizes) <= min(LARGEST_OLD_FILE, 1 << 20) and sum(sizes) <= TOTAL_CAP, (max(sizes), sum(sizes))
    assert all("attention_ref" in load_matrix(f)["README"] for f in MATRIX_FAMILIES)


def _check(got, ref, tol, what):
    err = np.abs(got - ref).max() if ref.size else 0.0
    assert err < tol, (what, err, tol)


@pytest.mark.parametrize("family,name", CASES, ids=[n for _, n in CASES])
def test_oracle_matches_reference_matrix(family, name):
    """oracle fwd / bwd == the reference's attention_ref (+ autograd) in fp32, the tolerances of test_oracle_cpu.py (2e-5 on out -- and on LSE --,
    5e-5 * max(1, max|ref|) on gradients)."""
    case = load_matrix(family)[name]
    m = matrix_meta(case)
    q, k, v, do = _inputs(case)
    rows = slice(None) if m["rows"] is None else m["rows"]
    args = (m["causal"], m["window"], m["softcap"], m["alibi"])
    if not m["packed"]:
        out, lse = orc.attention_fwd(q, k, v, None, *args)
        dq, dk, dv, _ = orc.attention_bwd(do, q, k, v, None, None, None, *args)
        _check(out[:, rows], case["out"], 2e-5, "out")
        fin = np.isfinite(case["lse"])
        assert np.array_equal(np.isposinf(lse[:, :, rows]), ~fin) and np.array_equal(np.isposinf(case["lse"]), ~fin)
        _check(lse[:, :, rows][fin], case["lse"][fin], 2e-5, "lse")
        for nm, got, ref in (("dq", dq[:, rows], case["dq"]), ("dk", dk, case["dk"]), ("dv", dv, case["dv"])):
            _check(got, ref, 5e-5 * max(1.0, np.abs(ref).max()), nm)
        return
    # the window of a packed batch is normalised once, by the batch's longest key sequence (what the varlen entry gets as max_seqlen_k), not per sequence: a bound
    # beyond ONE sequence's keys still binds it where that sequence has more rows than keys, as in the reference's construct_local_mask
    kw = dict(max_seqlen_k=int(case["kmask"].sum(1).max()))
    for b in range(m["B"]):
        lq, lk = int(case["qmask"][b].sum()), int(case["kmask"][b].sum())
        for nm, n in (("out", lq), ("dq", lq), ("dk", lk), ("dv", lk)):
            assert np.all(case[nm][b, n:] == 0), (nm, b)          # padded rows and keys: exact zeros
        if lq == 0 or lk == 0:
            assert all(np.all(case[nm][b] == 0) for nm in ("out", "dq", "dk", "dv")), b
            continue
        sl = lambda x, n: x[b:b + 1, :n]
        out, lse = orc.attention_fwd(sl(q, lq), sl(k, lk), sl(v, lk), None, *args, **kw)
        dq, dk, dv, _ = orc.attention_bwd(sl(do, lq), sl(q, lq), sl(k, lk), sl(v, lk), None, None, None, *args, **kw)
        _check(out, sl(case["out"], lq), 2e-5, ("out", b))
        ref_l = case["lse"][b:b + 1, :, :lq]
        fin = np.isfinite(ref_l)
        assert np.array_equal(np.isposinf(lse), ~fin)
        _check(lse[fin], ref_l[fin], 2e-5, ("lse", b))
        for nm, got, ref in (("dq", dq, sl(case["dq"], lq)), ("dk", dk, sl(case["dk"], lk)), ("dv", dv, sl(case["dv"], lk))):
            _check(got, ref, 5e-5 * max(1.0, np.abs(ref).max()), (nm, b))


@pytest.mark.parametrize("family,name", CASES, ids=[n for _, n in CASES])
def test_bound_is_met_by_the_rounded_reference(family, name):
    """The GPU module's bound must be satisfiable: the best a kernel can return is the fp32 reference rounded to the output dtype."""
    case = load_matrix(family)[name]
    for dtype, dn in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        for nm in ("out", "dq", "dk", "dv"):
            ref = torch.from_numpy(case[nm])
            err = float((ref.to(dtype).float() - ref).abs().max()) if ref.numel() else 0.0
            bound = matrix_bound(case, nm, dn, float(ref.abs().max()) if ref.numel() else 0.0)
            assert err <= bound, (nm, dn, err, bound)
