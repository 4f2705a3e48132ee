"""libfa_gfx950_combine.so without a GPU: the header, the ctypes mirror and the built library agree; every rule of the layout contract is answered with its error
code and a message naming the argument before anything touches a device (the pointers here are made-up addresses: a call that got past validation would
fault); the Python layer refuses what it must and its custom ops give the right fake shapes; the library is opened on first use only; and the golden fixture
of the reference's combine oracle loads and obeys the formula the GPU tests recompute."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from flash_attn_amd import _cabi_combine as cc
from flash_attn_amd import flash_attn_combine, merge_attn_states
from tests._combine_ref import combine_ref64, load_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "flash-attention_amd")
BASE = 0x7F0000000000          # a 16-byte aligned address that is never dereferenced
B, S, H, D, N = 2, 5, 4, 64, 3
GOLDEN = os.path.join(ROOT, "tests", "golden", "combine_ref_cases.npz")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "libfa_gfx950_combine.so")):
        subprocess.check_call([sys.executable, os.path.join(PKG, "build.py")])
    return cc.load()


def _params(n_sources=2, n0=N, n1=1, dt0=cc.FA_COMBINE_DTYPE_FP32, dt1=cc.FA_COMBINE_DTYPE_BF16, out_dt=cc.FA_COMBINE_DTYPE_BF16, b=B, s=S, h=H, d=D):
    """A valid call on dense tensors at made-up addresses: o (n, b, s, h, d), lse (n, b, h, s), out (b, s, h, d), lse (b, h, s)."""
    a = cc.FaCombineParams()
    a.n_sources, a.out_dtype, a.b, a.s, a.h, a.d, a.empty_lse_sign, a.path = n_sources, out_dt, b, s, h, d, 1, 0
    for i, (n, dt) in enumerate(((n0, dt0), (n1, dt1))[:n_sources]):
        t = a.src[i]
        t.o, t.lse, t.n_splits, t.dtype = BASE + (i << 36), BASE + (i << 36) + (1 << 34), n, dt
        t.o_split_stride, t.o_batch_stride, t.o_row_stride, t.o_head_stride = b * s * h * d, s * h * d, h * d, d
        t.lse_split_stride, t.lse_batch_stride, t.lse_row_stride, t.lse_head_stride = b * h * s, h * s, 1, s
    a.out, a.lse = BASE + (5 << 36), BASE + (6 << 36)
    a.out_batch_stride, a.out_row_stride, a.out_head_stride = s * h * d, h * d, d
    a.lse_batch_stride, a.lse_row_stride, a.lse_head_stride = h * s, 1, s
    return a


def _refused(lib, a, *words, code=-1):
    rc = lib.fa_combine(C.byref(a), None)
    msg = lib.fa_combine_last_error().decode()
    assert rc == code, (rc, msg)
    assert msg.startswith("fa_combine:") and all(w in msg for w in words), msg
    assert lib.fa_combine_last_kernel_name() == b""


def _declared_functions():
    hdr = open(os.path.join(ROOT, "include", "fa_gfx950_combine.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(fa_[a-z_0-9]+)\s*\(", hdr)))


def test_header_mirror_and_library_agree(lib):
    names = _declared_functions()
    assert set(names) == set(cc.EXPORTS), (names, cc.EXPORTS)
    raw = C.CDLL(cc.library_path())
    for n in names:
        assert hasattr(raw, n), n
    hdr = open(os.path.join(ROOT, "include", "fa_gfx950_combine.h")).read()
    for macro in ("FA_COMBINE_ABI_VERSION", "FA_COMBINE_MAX_SOURCES", "FA_COMBINE_MAX_SPLITS", "FA_COMBINE_ROWS_MAX_SPLITS"):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == getattr(cc, macro), macro
    assert lib.fa_combine_abi_version() == cc.FA_COMBINE_ABI_VERSION == 1
    assert cc.FA_COMBINE_MAX_SPLITS == 256
    assert lib.fa_sizeof_combine_source() == C.sizeof(cc.FaCombineSource)
    assert lib.fa_sizeof_combine_params() == C.sizeof(cc.FaCombineParams)
    enums = dict(re.findall(r"(FA_COMBINE_(?:DTYPE|PATH)_\w+) = (\d+)", hdr))
    assert enums and all(int(v) == getattr(cc, k) for k, v in enums.items()), enums


def test_ctypes_mirror_matches_c_structs(lib, tmp_path):
    """Field by field: a C program prints offsetof() of every member of both structs."""
    lines = []
    for cls in (cc.FaCombineSource, cc.FaCombineParams):
        for name, _ in cls._fields_:
            lines.append(f'  printf("{cls.__name__}.{name} %zu\\n", offsetof({cls.__name__}, {name}));')
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fa_gfx950_combine.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "offsets"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cls in (cc.FaCombineSource, cc.FaCombineParams):
        for name, _ in cls._fields_:
            assert int(got[f"{cls.__name__}.{name}"]) == getattr(cls, name).offset, (cls.__name__, name)


def test_call_wide_rules_are_refused(lib):
    _refused(lib, _params(n_sources=0), "n_sources = 0", "1 to 2")
    _refused(lib, _params(n_sources=3), "n_sources = 3")
    _refused(lib, _params(n0=0), "src[0].n_splits = 0", "at least 1")
    _refused(lib, _params(n0=200, n1=57), "n_splits", "257 partials", "FA_COMBINE_MAX_SPLITS = 256")
    _refused(lib, _params(n_sources=1, n0=257), "257 partials")
    _refused(lib, _params(dt1=2), "src[1].dtype", "fp16 (0), bf16 (1) or fp32 (3)")             # 2 is the main header's e4m3
    _refused(lib, _params(out_dt=4), "out_dtype")
    _refused(lib, _params(b=-1), "b, s and h", "negative")
    for d in (0, 4, 12, 520, 1024):
        _refused(lib, _params(d=d), f"d = {d}", "multiple of 8 in [8, 512]")
    a = _params()
    a.empty_lse_sign = 0
    _refused(lib, a, "empty_lse_sign", "+1 or -1")
    a = _params()
    a.path = 3
    _refused(lib, a, "path")
    _refused(lib, _params(b=1 << 16, s=1 << 14, h=2), "b * s * h", "2^31")
    rc = lib.fa_combine(None, None)
    assert rc == -1 and b"params is NULL" in lib.fa_combine_last_error()


@pytest.mark.parametrize("k", [0, 1])
def test_each_layout_rule_is_refused_per_source(lib, k):
    o, lse = f"src[{k}].o", f"src[{k}].lse"
    a = _params()
    a.src[k].o += 8
    _refused(lib, a, o, "16-byte aligned")
    a = _params()
    a.src[k].lse += 2
    _refused(lib, a, lse, "4-byte aligned")
    for field, name in (("o", o), ("lse", lse)):
        a = _params()
        setattr(a.src[k], field, None)
        _refused(lib, a, name, "non-NULL")
    bad = 2 if k == 0 else 4                     # source 0 is fp32 (4 elements per 16 bytes), source 1 bf16 (8)
    for which in ("batch", "row", "head") + (("split",) if k == 0 else ()):
        a = _params()
        setattr(a.src[k], f"o_{which}_stride", getattr(a.src[k], f"o_{which}_stride") + bad)
        _refused(lib, a, o, f"{which} stride", "multiple of 16 bytes")
        a = _params()
        setattr(a.src[k], f"o_{which}_stride", 0)                                     # an expanded input is accepted: the next rule is reached
        a.out += 4
        _refused(lib, a, "out must be", "16-byte aligned")
    a = _params()
    a.src[k].lse_row_stride, a.src[k].lse_head_stride = 7, 3                           # lse: any element strides -- nothing to refuse; the next rule is reached
    a.out += 4
    _refused(lib, a, "out", "16-byte aligned")


def test_output_rules_are_refused(lib):
    a = _params()
    a.out = None
    _refused(lib, a, "out", "non-NULL")
    a = _params()
    a.lse += 1
    _refused(lib, a, "lse", "4-byte aligned")
    for which in ("batch", "row", "head"):
        a = _params()
        setattr(a, f"out_{which}_stride", getattr(a, f"out_{which}_stride") + 4)       # bf16: 8 bytes off
        _refused(lib, a, "out", f"{which} stride", "multiple of 16 bytes")
        a = _params()
        setattr(a, f"out_{which}_stride", 0)
        _refused(lib, a, "out", f"{which} stride", "must not be 0")
        a = _params()
        setattr(a, f"lse_{which}_stride", 0)
        _refused(lib, a, "lse", f"{which} stride", "must not be 0")


def test_a_call_without_rows_succeeds_and_size_one_dimensions_take_any_stride(lib):
    for zero in ("b", "s", "h"):
        a = _params(**{zero: 0})
        a.out = a.lse = None                                                           # an empty torch tensor has a null data pointer
        a.src[0].o = a.src[1].lse = None
        assert lib.fa_combine(C.byref(a), None) == 0 and lib.fa_combine_last_error() == b"" and lib.fa_combine_last_kernel_name() == b""
    a = _params(n_sources=1, n0=1, b=1, s=1, h=1)                                      # no stride is ever used ... until the next check fails
    t = a.src[0]
    t.o_split_stride, t.o_batch_stride, t.o_row_stride, t.o_head_stride = 1, 3, 5, 7
    a.out_batch_stride, a.out_row_stride, a.out_head_stride = 0, 1, 9
    a.lse_batch_stride = a.lse_row_stride = a.lse_head_stride = 0
    a.out += 8
    _refused(lib, a, "out", "16-byte aligned")
    a.out -= 8
    a.s = 2                                                                            # ... and as soon as the dimension has two elements, its stride counts
    _refused(lib, a, "src[0].o", "row stride")


def test_missing_combine_library_fails_on_first_use_only(tmp_path):
    code = ("import flash_attn_amd\n"
            "from flash_attn_amd import flash_attn_combine, merge_attn_states, _cabi, _cabi_combine\n"
            "_cabi.load()\n"
            "try:\n    _cabi_combine.load()\nexcept ImportError as e:\n    print('ImportError:', e)\n")
    env = dict(os.environ, FA_GFX950_COMBINE_LIB=str(tmp_path / "absent.so"), PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ImportError:" in r.stdout and "absent.so not found" in r.stdout and "build.py" in r.stdout, r.stdout


def test_python_checks_refuse_before_the_library_is_needed():
    o, l = torch.zeros(2, 1, 3, 2, 16), torch.zeros(2, 1, 3, 2)
    with pytest.raises(RuntimeError, match="has no backward"):
        flash_attn_combine(o.clone().requires_grad_(True), l)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="CUDA device"):
            flash_attn_combine(o.clone().requires_grad_(True), l)                      # (grad mode off: the next check is reached)
    with pytest.raises(RuntimeError, match="lse_partial must have shape"):
        flash_attn_combine(o, l[:, :, :2])
    with pytest.raises(RuntimeError, match="num_splits, batch"):
        flash_attn_combine(o[0, 0], l[0, 0])
    with pytest.raises(RuntimeError, match="fp32, bf16 or fp16"):
        flash_attn_combine(o.double(), l)
    with pytest.raises(RuntimeError, match="lse_partial must be fp32"):
        flash_attn_combine(o, l.half())
    with pytest.raises(RuntimeError, match="out_dtype"):
        flash_attn_combine(o, l, out_dtype=torch.float64)
    a, la = torch.zeros(1, 3, 2, 16, dtype=torch.bfloat16), torch.zeros(1, 2, 3)
    with pytest.raises(RuntimeError, match="has no backward"):
        merge_attn_states(a, la.clone().requires_grad_(True), a, la)
    with pytest.raises(RuntimeError, match="CUDA device"):
        merge_attn_states(a, la, a, la)
    with pytest.raises(RuntimeError, match=r"lse_b must have shape \(.., heads, seqlen\)"):
        merge_attn_states(a, la, a, la.transpose(1, 2))
    with pytest.raises(RuntimeError, match="out_b must have the shape of out_a"):
        merge_attn_states(a, la, a[:, :2], la)
    with pytest.raises(RuntimeError, match="lse must be fp32"):
        merge_attn_states(a, la, a, la, lse=la.half())
    with FakeTensorMode():
        c = torch.empty(300, 1, 2, 2, 16, device="cuda")
        with pytest.raises(RuntimeError, match=r"num_splits must be in \[1, 256\]"):
            flash_attn_combine(c, c[..., 0])
        c = torch.empty(2, 1, 2, 2, 12, device="cuda")
        with pytest.raises(RuntimeError, match="multiple of 8"):
            flash_attn_combine(c, c[..., 0])
        with pytest.raises(RuntimeError, match="contiguous last dimension"):
            merge_attn_states(torch.empty(1, 3, 16, 2, device="cuda").transpose(2, 3), torch.empty(1, 2, 3, device="cuda"),
                              torch.empty(1, 3, 2, 16, device="cuda"), torch.empty(1, 2, 3, device="cuda"))


def test_ops_are_registered_and_fake_implementations_give_the_shapes():
    ns = torch.ops.flash_attn_amd
    assert "Tensor(a2!)? out" in str(ns._flash_attn_combine.default._schema), ns._flash_attn_combine.default._schema
    schema = str(ns._merge_attn_states.default._schema)
    assert "Tensor(a4!)? out" in schema and "Tensor(a5!)? lse" in schema, schema
    with FakeTensorMode():
        dev = "cuda"
        op = torch.empty(7, 3, 113, 4, 64, device=dev, dtype=torch.float32)
        lp = torch.empty(7, 3, 4, 113, device=dev).transpose(-1, -2)
        out, lse = flash_attn_combine(op, lp)
        assert out.shape == (3, 113, 4, 64) and out.dtype == torch.float32 and out.is_contiguous() and out.device.type == "cuda"
        assert lse.shape == (3, 113, 4) and lse.dtype == torch.float32 and lse.stride() == (4 * 113, 1, 113)      # the transpose of a contiguous (B, H, L)
        out, lse = flash_attn_combine(op, lp, out_dtype=torch.bfloat16, return_lse=False)
        assert out.dtype == torch.bfloat16 and lse is None
        given = torch.empty(3, 113, 4, 64, device=dev, dtype=torch.float16)
        out, lse = flash_attn_combine(op.to(torch.bfloat16), lp, out=given)
        assert out is given and lse.shape == (3, 113, 4)
        with pytest.raises(RuntimeError, match="out has dtype"):
            flash_attn_combine(op, lp, out=given, out_dtype=torch.bfloat16)
        op, lp = torch.empty(5, 230, 4, 128, device=dev, dtype=torch.float16), torch.empty(5, 230, 4, device=dev)     # packed
        out, lse = flash_attn_combine(op, lp)
        assert out.shape == (230, 4, 128) and out.dtype == torch.float16 and lse.shape == (230, 4) and lse.stride() == (1, 230)
        a, la = torch.empty(2, 100, 4, 128, device=dev, dtype=torch.bfloat16), torch.empty(2, 4, 100, device=dev)
        b = torch.empty(2, 100, 4, 128, device=dev, dtype=torch.float32)
        out, lse = merge_attn_states(a, la, b, la)
        assert out.shape == a.shape and out.dtype == torch.bfloat16 and out.is_contiguous() and lse.shape == (2, 4, 100) and lse.is_contiguous()
        out, lse = merge_attn_states(b, la, a, la)
        assert out.dtype == torch.float32
        out, lse = merge_attn_states(a, la, b, la, out=b, lse=la)                      # in place on the second operand's buffers is fine for shapes
        assert out is b and lse is la
        a, la = torch.empty(230, 4, 128, device=dev, dtype=torch.float16), torch.empty(4, 230, device=dev)            # packed
        out, lse = merge_attn_states(a, la, a, la)
        assert out.shape == (230, 4, 128) and lse.shape == (4, 230) and lse.is_contiguous()


def test_golden_fixture_obeys_its_formula():
    """The stored results of the reference's oracle equal the float64 recomputation the GPU tests use for 16-bit partials, so both references are one.

    What the fixture can and cannot catch, shown on its own arrays:
      * a merge that does not mask empty partials (exp(lse_i - lse) with lse = -inf on a row without a live split, the S = 1 case) is NaN there: caught;
      * the same values with this library's marker, +inf, instead of -inf: a merge that takes +inf as live returns lse = +inf and NaN rows wherever a row has
        ONE empty partial -- every case with B // 3 batch entries of half-empty splits: caught by the NaN test of the GPU suite, which uses both markers;
      * a dropped max-subtraction is NOT caught here: the reference draws lse ~ N(0, 1), where exp() neither overflows nor underflows; the GPU range test
        (lse = 30 randn +- 80) is the one that fails for it -- in fp32 exp(80 + ...) is inf."""
    cases = load_cases(GOLDEN)
    assert len(cases) >= 12
    seen = {k: set() for k in "sld"}
    for name, c in cases.items():
        s, l, d, h = (int(x[1:]) for x in name.split("_"))
        seen["s"].add(s), seen["l"].add(l), seen["d"].add(d)
        assert c["out_partial"].shape == (s, 3, l, h, d) and c["lse_partial"].shape == (s, 3, l, h) and c["out_partial"].dtype == np.float32
        assert np.isneginf(c["lse_partial"][s // 2:, :1]).all() and np.isfinite(c["lse_partial"][:, 1:]).all() and np.isfinite(c["lse_partial"][:s // 2]).all()
        out, lse = combine_ref64(c["out_partial"], c["lse_partial"])
        assert np.array_equal(np.isneginf(lse), np.isneginf(c["lse"])) and np.isfinite(c["out"]).all()
        assert np.allclose(lse, c["lse"], atol=2e-6, rtol=2e-6) and np.abs(out - c["out"]).max() < 2e-5, name     # (fp32 sums of up to 256 terms of |o| < 5)
        if s == 1:
            assert np.isneginf(c["lse"][0]).all() and (c["out"][0] == 0).all()                                     # whole batch entries without a live split
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            lp, op = c["lse_partial"], c["out_partial"]
            naive_lse = np.log(np.exp(lp).sum(0))                                                                    # no max-subtraction, no mask
            naive = (np.exp(lp - naive_lse)[..., None] * op).sum(0)
            assert np.isnan(naive).any() == (s == 1), name                                                           # unmasked: NaN exactly where no split is live
            assert np.allclose(naive[1:], c["out"][1:], atol=1e-5)                                                   # ... and the dropped max goes unnoticed
            plus = np.where(np.isneginf(lp), np.inf, lp)                                                             # this library's marker, taken as live
            bad = (np.exp(plus - np.log(np.exp(plus).sum(0)))[..., None] * op).sum(0)
            assert np.isnan(bad[0]).all() and np.isfinite(bad[1:]).all(), name
    assert seen["s"] == {1, 2, 3, 5, 17, 64, 65, 133, 256} and seen["l"] == {1, 3, 113} and seen["d"] == {8, 40, 64, 96, 128, 192, 256, 512}
    assert os.path.getsize(GOLDEN) < 1_000_000


def test_kernels_use_no_scratch(lib, monkeypatch):
    """Both kernels keep their partials in flight in registers: no private segment, no spills; and the library holds the two kernels the design names."""
    from tests import _kernel_census as kc
    monkeypatch.setattr(kc, "LIB", cc.library_path())
    meta = kc.kernel_metadata()
    assert sorted(re.match(r"_ZN2fc\d+(fa_combine_\w+?_kernel)", n).group(1) for n in meta) == ["fa_combine_rows_kernel", "fa_combine_splits_kernel"], list(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)          # two workgroups of 256 threads per SIMD set at least
