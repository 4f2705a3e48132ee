"""libfa_gfx950_sink.so without a GPU: the header, the ctypes mirror and the built library agree; every rule of the layout contract is answered with its error
code and a message naming the argument before anything touches a device (the pointers here are made-up addresses: a call that got past validation would
fault); the Python layer refuses what it must and its custom ops give the right fake shapes; the library is opened on first use only; and the fixture of the
reference's oracle leaves the kernels room -- the torch stand-in with their roundings stays within half of each of the reference's allowances -- while the same
comparison reports every one of five planted mistakes."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from flash_attn_amd import _cabi_sink as cs
from flash_attn_amd import apply_attn_sink, flash_attn_sink_func, flash_attn_varlen_sink_func, flash_attn_with_kvcache_sink
from tests import _sink_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "flash-attention_amd")
BASE = 0x7F0000000000          # a 16-byte aligned address that is never dereferenced
B, S, H, D = 2, 5, 4, 64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "libfa_gfx950_sink.so")):
        subprocess.check_call([sys.executable, os.path.join(PKG, "build.py")])
    return cs.load()


def _apply(b=B, s=S, h=H, d=D, dtype=cs.FA_SINK_DTYPE_BF16, sink_dtype=cs.FA_SINK_DTYPE_FP32, in_place=False):
    """A valid call on dense tensors at made-up addresses: out (b, s, h, d), lse (b, h, s), sink (h)."""
    a = cs.FaSinkApplyParams()
    a.b, a.s, a.h, a.d, a.dtype, a.sink_dtype = b, s, h, d, dtype, sink_dtype
    a.out_in, a.lse_in, a.sink = BASE, BASE + (1 << 36), BASE + (2 << 36)
    a.out, a.lse, a.lse_bwd = (a.out_in, a.lse_in, BASE + (5 << 36)) if in_place else (BASE + (3 << 36), BASE + (4 << 36), BASE + (5 << 36))
    for t in ("out_in", "out"):
        setattr(a, t + "_batch_stride", s * h * d), setattr(a, t + "_row_stride", h * d), setattr(a, t + "_head_stride", d)
    for t in ("lse_in", "lse", "lse_bwd"):
        setattr(a, t + "_batch_stride", h * s), setattr(a, t + "_row_stride", 1), setattr(a, t + "_head_stride", s)
    a.sink_stride = 1
    return a


def _dsink(b=B, s=S, h=H, sink_dtype=cs.FA_SINK_DTYPE_FP32, ws=None):
    a = cs.FaSinkDsinkParams()
    a.b, a.s, a.h, a.sink_dtype = b, s, h, sink_dtype
    a.softmax_d, a.lse_bwd, a.sink, a.dsink, a.workspace = BASE, BASE + (1 << 36), BASE + (2 << 36), BASE + (3 << 36), BASE + (4 << 36)
    for t in ("softmax_d", "lse_bwd"):
        setattr(a, t + "_batch_stride", h * s), setattr(a, t + "_row_stride", 1), setattr(a, t + "_head_stride", s)
    a.sink_stride = a.dsink_stride = 1
    a.workspace_bytes = 4 * h * cs.FA_SINK_DSINK_MAX_BLOCKS if ws is None else ws
    return a


def _refused(lib, fn, a, *words, code=-1):
    rc = getattr(lib, fn)(C.byref(a), None)
    msg = lib.fa_sink_last_error().decode()
    assert rc == code, (rc, msg)
    assert msg.startswith(fn + ":") and all(w in msg for w in words), msg
    assert lib.fa_sink_last_kernel_name() == b""


def _header():
    return open(os.path.join(ROOT, "include", "fa_gfx950_sink.h")).read()


def test_header_mirror_and_library_agree(lib):
    hdr = _header()
    names = sorted(set(re.findall(r"\b(fa_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert set(names) == set(cs.EXPORTS), (names, cs.EXPORTS)
    raw = C.CDLL(cs.library_path())
    for n in names:
        assert hasattr(raw, n), n
    for macro in ("FA_SINK_ABI_VERSION", "FA_SINK_DSINK_MAX_BLOCKS"):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == getattr(cs, macro), macro
    assert lib.fa_sink_abi_version() == cs.FA_SINK_ABI_VERSION == 1
    assert lib.fa_sink_sizeof_apply_params() == C.sizeof(cs.FaSinkApplyParams)
    assert lib.fa_sink_sizeof_dsink_params() == C.sizeof(cs.FaSinkDsinkParams)
    enums = dict(re.findall(r"(FA_SINK_DTYPE_\w+) = (\d+)", hdr))
    assert len(enums) == 3 and all(int(v) == getattr(cs, k) for k, v in enums.items()), enums


def test_ctypes_mirror_matches_c_structs(lib, tmp_path):
    """Field by field: a C program prints offsetof() of every member of both structs."""
    lines = []
    for cls in (cs.FaSinkApplyParams, cs.FaSinkDsinkParams):
        for name, _ in cls._fields_:
            lines.append(f'  printf("{cls.__name__}.{name} %zu\\n", offsetof({cls.__name__}, {name}));')
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fa_gfx950_sink.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "offsets"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cls in (cs.FaSinkApplyParams, cs.FaSinkDsinkParams):
        for name, _ in cls._fields_:
            assert int(got[f"{cls.__name__}.{name}"]) == getattr(cls, name).offset, (cls.__name__, name)


def test_apply_call_wide_rules_are_refused(lib):
    fn = "fa_sink_apply"
    assert lib.fa_sink_apply(None, None) == -1 and b"params is NULL" in lib.fa_sink_last_error()
    _refused(lib, fn, _apply(dtype=3), "dtype must be fp16 (0) or bf16 (1)")                   # fp32 is a dtype of the sink only
    _refused(lib, fn, _apply(dtype=2), "dtype")
    for bad in (2, 4, -1):
        _refused(lib, fn, _apply(sink_dtype=bad), "sink_dtype", "fp16 (0), bf16 (1) or fp32 (3)")
    _refused(lib, fn, _apply(b=-1), "b, s and h", "negative")
    for d in (0, 4, 12, 520, 1024):
        _refused(lib, fn, _apply(d=d), f"d = {d}", "multiple of 8 in [8, 512]")
    _refused(lib, fn, _apply(b=1 << 16, s=1 << 14, h=2), "b * s * h", "2^31")


def test_apply_pointer_and_stride_rules_are_refused(lib):
    fn = "fa_sink_apply"
    for field in ("out_in", "lse_in", "sink", "out", "lse"):
        a = _apply()
        setattr(a, field, None)
        _refused(lib, fn, a, field + " must be non-NULL")
    for field in ("out_in", "out"):
        a = _apply()
        setattr(a, field, getattr(a, field) + 8)                                               # a pointer 8 bytes off
        _refused(lib, fn, a, field + " must be", "16-byte aligned")
    for field in ("lse_in", "lse", "lse_bwd"):
        a = _apply()
        setattr(a, field, getattr(a, field) + 2)
        _refused(lib, fn, a, field + " must be", "4-byte aligned")
    a = _apply()
    a.sink += 2
    _refused(lib, fn, a, "sink must be", "4-byte aligned")
    a = _apply(sink_dtype=cs.FA_SINK_DTYPE_BF16)
    a.sink += 2                                                                                # ... a 16-bit sink is aligned to 2: the next rule is reached
    a.out += 4
    _refused(lib, fn, a, "out must be", "16-byte aligned")
    for tensor in ("out_in", "out"):
        for which in ("batch", "row", "head"):
            a = _apply()
            f = f"{tensor}_{which}_stride"
            setattr(a, f, getattr(a, f) + 1)                                                   # an odd stride
            _refused(lib, fn, a, tensor + ":", f"{which} stride", "multiple of 16 bytes")
            a = _apply()
            setattr(a, f, getattr(a, f) + 4)                                                   # 8 bytes off
            _refused(lib, fn, a, tensor + ":", f"{which} stride", "multiple of 16 bytes")
    for which in ("batch", "row", "head"):
        a = _apply()
        setattr(a, f"out_in_{which}_stride", 0)                                                # an expanded input is accepted: the next rule is reached
        a.lse_row_stride = 0
        _refused(lib, fn, a, "lse:", "row stride", "must not be 0")
        for tensor in ("out", "lse", "lse_bwd"):
            a = _apply()
            setattr(a, f"{tensor}_{which}_stride", 0)
            _refused(lib, fn, a, tensor + ":", f"{which} stride", "must not be 0")
    a = _apply()
    a.lse_in_row_stride, a.lse_in_head_stride = 7, 3                                           # lse: any element strides -- nothing to refuse; the next rule is reached
    a.lse_bwd_head_stride = 0
    _refused(lib, fn, a, "lse_bwd:", "head stride")


def test_apply_aliasing_exact_is_allowed_partial_overlap_is_refused(lib):
    fn = "fa_sink_apply"
    a = _apply(in_place=True)                                                                  # out = out_in, lse = lse_in: valid -- shown by the NEXT rule answering
    a.lse_bwd = a.lse
    _refused(lib, fn, a, "lse_bwd overlaps lse")
    a = _apply(in_place=True)
    a.lse_bwd = None                                                                           # optional
    a.lse_in += 4                                                                              # lse one element off lse_in
    _refused(lib, fn, a, "lse overlaps lse_in", "same pointer and strides")
    a = _apply(in_place=True)
    a.lse_head_stride, a.lse_row_stride = 1, H                                                 # same pointer, other strides
    _refused(lib, fn, a, "lse overlaps lse_in")
    a = _apply(in_place=True)
    a.out = a.out_in + 16 * D                                                                  # out eight rows into out_in
    _refused(lib, fn, a, "out overlaps out_in", "same pointer and strides")
    a = _apply()
    a.lse_bwd = a.lse_in                                                                       # lse_bwd exactly lse_in is allowed: the next rule answers
    a.lse = a.lse_in + 4
    _refused(lib, fn, a, "lse overlaps lse_in")
    a = _apply()
    a.lse = a.out + 64
    _refused(lib, fn, a, "overlap")
    a = _apply()
    a.lse_bwd = a.out_in + 32
    _refused(lib, fn, a, "lse_bwd overlaps out / out_in")


def test_dsink_rules_are_refused(lib):
    fn = "fa_sink_dsink"
    assert lib.fa_sink_dsink(None, None) == -1 and b"params is NULL" in lib.fa_sink_last_error()
    _refused(lib, fn, _dsink(sink_dtype=2), "sink_dtype")
    _refused(lib, fn, _dsink(s=-1), "negative")
    _refused(lib, fn, _dsink(b=1 << 16, s=1 << 14, h=2), "2^31")
    for field in ("softmax_d", "lse_bwd", "sink", "dsink", "workspace"):
        a = _dsink()
        setattr(a, field, None)
        _refused(lib, fn, a, field + " must be non-NULL")
        a = _dsink()
        setattr(a, field, getattr(a, field) + 2)
        _refused(lib, fn, a, field + " must be 4-byte aligned")
    a = _dsink()
    a.dsink_stride = 0
    _refused(lib, fn, a, "dsink:", "head stride", "must not be 0")
    # the workspace: h * min(64, ceil(b * s / 1024)) floats
    for b, s, h, blocks in ((B, S, H, 1), (1, 1024, 3, 1), (1, 1025, 3, 2), (4, 4096, 32, 16), (8, 65536, 2, 64)):
        a = _dsink(b=b, s=s, h=h)
        need = lib.fa_sink_dsink_workspace_bytes(C.byref(a))
        assert need == 4 * h * blocks, (b, s, h, need)
        _refused(lib, fn, _dsink(b=b, s=s, h=h, ws=need - 1), "workspace_bytes", "too small", str(need))
        _refused(lib, fn, _dsink(b=b, s=s, h=h, ws=0), "workspace_bytes = 0", "too small")
    assert lib.fa_sink_dsink_workspace_bytes(None) == 0 and lib.fa_sink_dsink_workspace_bytes(C.byref(_dsink(h=0))) == 0


def test_calls_without_rows_succeed_and_size_one_dimensions_take_any_stride(lib):
    for zero in ("b", "s", "h"):
        a = _apply(**{zero: 0})
        a.out = a.lse = a.out_in = a.lse_in = a.sink = None                                    # an empty torch tensor has a null data pointer
        assert lib.fa_sink_apply(C.byref(a), None) == 0 and lib.fa_sink_last_error() == b"" and lib.fa_sink_last_kernel_name() == b""
    a = _dsink(h=0)
    a.dsink = a.softmax_d = None
    assert lib.fa_sink_dsink(C.byref(a), None) == 0 and lib.fa_sink_last_kernel_name() == b""
    a = _apply(b=1, s=1, h=1)                                                                  # no stride is ever used ... until the next check fails
    a.out_in_batch_stride, a.out_in_row_stride, a.out_in_head_stride = 1, 3, 5
    a.out_batch_stride, a.out_row_stride, a.out_head_stride = 0, 1, 9
    a.lse_batch_stride = a.lse_row_stride = a.lse_head_stride = 0
    a.out += 8
    _refused(lib, "fa_sink_apply", a, "out must be", "16-byte aligned")
    a.out -= 8
    a.s = 2                                                                                    # ... and as soon as the dimension has two elements, its stride counts
    _refused(lib, "fa_sink_apply", a, "out_in:", "row stride")


def test_missing_sink_library_fails_on_first_use_only(tmp_path):
    code = ("import flash_attn_amd\n"
            "from flash_attn_amd import apply_attn_sink, flash_attn_sink_func, flash_attn_varlen_sink_func, flash_attn_with_kvcache_sink, _cabi, _cabi_sink\n"
            "_cabi.load()\n"
            "try:\n    _cabi_sink.load()\nexcept ImportError as e:\n    print('ImportError:', e)\n")
    env = dict(os.environ, FA_GFX950_SINK_LIB=str(tmp_path / "absent.so"), PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ImportError:" in r.stdout and "absent.so not found" in r.stdout and "build.py" in r.stdout, r.stdout


def test_python_checks_refuse_before_the_library_is_needed():
    bf = torch.bfloat16
    o, l, s = torch.zeros(1, 3, 2, 16, dtype=bf), torch.zeros(1, 2, 3), torch.zeros(2)
    for bad in ((o.clone().requires_grad_(True), l, s), (o, l.clone().requires_grad_(True), s), (o, l, s.clone().requires_grad_(True))):
        with pytest.raises(RuntimeError, match="has no backward.*flash_attn_sink_func"):
            apply_attn_sink(*bad)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="CUDA device"):
            apply_attn_sink(o, l, s.clone().requires_grad_(True))                              # (grad mode off: the next check is reached)
    with pytest.raises(RuntimeError, match=r"lse must have shape \(.., heads, seqlen\)"):
        apply_attn_sink(o, l.transpose(1, 2), s)
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        apply_attn_sink(o.float(), l, s)
    with pytest.raises(RuntimeError, match="lse must be fp32"):
        apply_attn_sink(o, l.half(), s)
    with pytest.raises(RuntimeError, match="out_ must have the shape and dtype of out"):
        apply_attn_sink(o, l, s, out_=o.half())
    with pytest.raises(RuntimeError, match=r"learnable_sink must have shape \(nheads_q,\) = \(2,\)"):
        apply_attn_sink(o, l, torch.zeros(3))
    with pytest.raises(RuntimeError, match="learnable_sink must be fp32, bf16 or fp16"):
        apply_attn_sink(o, l, s.double())
    with pytest.raises(RuntimeError, match="learnable_sink must be on the device"):
        apply_attn_sink(o, l, s.to("meta"))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        apply_attn_sink(torch.zeros(1, 3, 2, 12, dtype=bf), l, s)
    q, k = torch.zeros(1, 3, 4, 16, dtype=bf), torch.zeros(1, 5, 2, 16, dtype=bf)
    cu = torch.tensor([0, 3], dtype=torch.int32)
    fixed = lambda sink, **kw: flash_attn_sink_func(q, k, k, sink, **kw)
    packed = lambda sink, **kw: flash_attn_varlen_sink_func(q[0], k[0], k[0], sink, cu, cu, 3, 5, **kw)
    for call, name in ((fixed, "flash_attn_sink_func"), (packed, "flash_attn_varlen_sink_func")):
        with pytest.raises(RuntimeError, match=name + ": dropout is not supported"):
            call(torch.zeros(4), dropout_p=0.1)
        with pytest.raises(RuntimeError, match=name + r": learnable_sink must have shape \(nheads_q,\) = \(4,\)"):
            call(torch.zeros(2))                                                               # per KV head: refused
        with pytest.raises(RuntimeError, match=name + ": learnable_sink must have shape"):
            call(torch.zeros(4, 1))
        with pytest.raises(RuntimeError, match=name + ": learnable_sink must be fp32, bf16 or fp16"):
            call(torch.zeros(4, dtype=torch.float64))
        with pytest.raises(RuntimeError, match=name + ": learnable_sink must be on the device"):
            call(torch.zeros(4, device="meta"))
        with pytest.raises(RuntimeError, match=name + ": learnable_sink must be a tensor"):
            call(None)
    q8 = q.to(torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match="flash_attn_sink_func: float8_e4m3fn"):
        flash_attn_sink_func(q8, k.to(torch.float8_e4m3fn), k.to(torch.float8_e4m3fn), torch.zeros(4))
    with pytest.raises(RuntimeError, match="flash_attn_varlen_sink_func: float8_e4m3fn"):
        flash_attn_varlen_sink_func(q8[0], k[0], k[0], torch.zeros(4), cu, cu, 3, 5)
    with pytest.raises(RuntimeError, match=r"flash_attn_with_kvcache_sink: learnable_sink must have shape \(nheads_q,\) = \(4,\)"):
        flash_attn_with_kvcache_sink(q, k, k, torch.zeros(2))
    with FakeTensorMode():
        with pytest.raises(RuntimeError, match="contiguous last dimension"):
            apply_attn_sink(torch.empty(1, 3, 16, 2, device="cuda", dtype=bf).transpose(2, 3), torch.empty(1, 2, 3, device="cuda"), torch.empty(2, device="cuda"))


def test_ops_are_registered_and_fake_implementations_give_the_shapes():
    ns = torch.ops.flash_attn_amd
    schema = str(ns._attn_sink_apply.default._schema)
    assert "Tensor(a3!)? out_" in schema and "Tensor(a4!)? lse_" in schema and "Tensor out," in schema and "Tensor lse," in schema, schema   # inputs only read
    schema = str(ns._attn_sink_apply_.default._schema)
    assert "Tensor(a0!) out" in schema and "Tensor(a1!) lse" in schema and schema.endswith("-> Tensor"), schema                      # the in-place op
    assert str(ns._attn_sink_dsink.default._schema).endswith("-> Tensor"), ns._attn_sink_dsink.default._schema
    with FakeTensorMode():
        dev = "cuda"
        for dt in (torch.bfloat16, torch.float16):
            o, l, s = torch.empty(2, 100, 4, 128, device=dev, dtype=dt), torch.empty(2, 4, 100, device=dev), torch.empty(4, device=dev, dtype=dt)
            out, lse = apply_attn_sink(o, l, s)
            assert out.shape == o.shape and out.dtype == dt and out.is_contiguous() and lse.shape == (2, 4, 100) and lse.dtype == torch.float32 and lse.is_contiguous()
            out, lse = apply_attn_sink(o, l, s, out_=o, lse_=l)                                # in place
            assert out is o and lse is l
            given = torch.empty_like(o)
            out, lse = apply_attn_sink(o, l, s, out_=given)
            assert out is given and lse.shape == (2, 4, 100) and lse is not l
        o, l, s = torch.empty(230, 4, 64, device=dev, dtype=torch.float16), torch.empty(4, 230, device=dev), torch.empty(4, device=dev)          # packed
        out, lse = apply_attn_sink(o, l, s)
        assert out.shape == (230, 4, 64) and lse.shape == (4, 230) and lse.is_contiguous()
        c = ns._attn_sink_apply_(o, l, s, True)                                               # the autograd functions' call: in place, plus lse_bwd
        assert c.shape == (4, 230) and c.dtype == torch.float32 and ns._attn_sink_apply_(o, l, s, False).numel() == 0
        l2 = torch.empty_like(l)
        assert ns._attn_sink_apply_out_(o, l, s, l2) is None                                  # out in place, lse' to another tensor: lse is only read
        assert "Tensor lse," in str(ns._attn_sink_apply_out_.default._schema) and "Tensor(a3!) lse_" in str(ns._attn_sink_apply_out_.default._schema)
        out, lse = apply_attn_sink(o, l, s, out_=o, lse_=l2)
        assert out is o and lse is l2
        out, lse = apply_attn_sink(o, l, s, out_=o)
        assert out is o and lse is not l and lse.shape == l.shape
        out, lse = apply_attn_sink(o, l, s, lse_=l)
        assert out is not o and out.shape == o.shape and lse is l
        a, b, c = ns._attn_sink_apply(o, l, s, None, None, False)
        assert a.shape == o.shape and a.dtype == o.dtype and b.shape == l.shape and c.numel() == 0
        a, b, c = ns._attn_sink_apply(o, l, s, torch.empty_like(o), None, True)
        assert a.numel() == 0 and b.shape == l.shape and c.shape == l.shape
        for shape in ((3, 5, 77), (5, 230)):
            ds = ns._attn_sink_dsink(torch.empty(shape, device=dev), torch.empty(shape, device=dev), torch.empty(5, device=dev, dtype=torch.bfloat16))
            assert ds.shape == (5,) and ds.dtype == torch.float32


def test_formulas_in_float64_agree_with_a_direct_softmax():
    """apply_ref64 / dsink_ref64 against a softmax over [scores, sink] written out, finite differences for dsink."""
    g = torch.Generator().manual_seed(5)
    Hh, Sq, Sk, Dd = 3, 7, 11, 8
    sc, v, do = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((Hh, Sq, Sk), (Hh, Sk, Dd), (Sq, Hh, Dd)))
    sc[:, 2] = -math.inf                                                                       # a row without a key
    sink = torch.tensor([0.3, -math.inf, 2.0], dtype=torch.float64)
    lse = torch.logsumexp(sc, -1)
    out = torch.einsum("hts,hsd->thd", torch.softmax(sc, -1).nan_to_num(0.0), v)
    out[2] = math.nan                                                                          # never multiplied
    o2, l2, lb = sr.apply_ref64(out, torch.where(torch.isinf(lse), torch.full_like(lse, math.inf), lse), sink)

    def direct(s):
        full = torch.cat([sc, s[:, None, None].expand(Hh, Sq, 1)], -1)
        return torch.einsum("hts,hsd->thd", torch.softmax(full, -1)[..., :-1].nan_to_num(0.0), v), torch.logsumexp(full, -1)

    od, ld = direct(sink)
    assert np.allclose(o2, od.numpy(), atol=1e-14) and (o2[2] == 0).all()
    assert np.allclose(l2[[0, 2]], ld[[0, 2]].numpy(), atol=1e-14) and np.array_equal(l2[1, [0, 1, 3]], lse[1, [0, 1, 3]].numpy()) and l2[1, 2] == math.inf
    assert np.isposinf(lb[:, 2]).all() and np.array_equal(lb[:, :2], l2[:, :2])
    delta = np.nansum(do.numpy() * o2, -1).T                                                   # (H, Sq)
    delta[:, 2] = math.nan                                                                     # unwritten on the row without a key
    ds, _ = sr.dsink_ref64(delta, lb, sink)
    eps = 1e-6
    for h in (0, 2):
        e = torch.zeros(Hh, dtype=torch.float64)
        e[h] = eps
        fd = float(((direct(sink + e)[0] - direct(sink - e)[0]) * do).sum()) / (2 * eps)
        assert abs(ds[h] - fd) < 1e-8, (h, ds[h], fd)
    assert ds[1] == 0


@pytest.fixture(scope="module")
def cases():
    c = sr.load_cases()
    assert len(c) == 12 and all(os.path.getsize(p) < (1 << 20) for p in sr.fixture_files())
    return c


def test_fixture_covers_what_it_must(cases):
    metas = {n: sr.case_meta(c) for n, c in cases.items()}
    assert {m["D"] for m in metas.values()} >= {40, 64, 128, 256}
    assert {m["H"] // m["Hk"] for m in metas.values()} >= {1, 2, 4, 8} and any(m["Hk"] == 1 and m["H"] > 1 for m in metas.values())
    assert any(m["softcap"] == 30.0 for m in metas.values()) and any(m["window"] == (31, 0) for m in metas.values())
    assert any(not m["causal"] and m["window"] == (-1, -1) for m in metas.values())
    assert any(m["qlens"] == [1] and m["klens"] == [515] for m in metas.values())
    assert sum(m["packed"] for m in metas.values()) == 2 and any(m["packed"] and 0 in m["qlens"] for m in metas.values())
    assert any(m["causal"] and m["qlens"][0] > m["klens"][0] for m in metas.values()) and any(m["causal"] and m["qlens"][0] < m["klens"][0] for m in metas.values())
    lens = {x for m in metas.values() for x in m["qlens"] + m["klens"]}
    assert {113, 200, 257} <= lens and max(lens - {515}) <= 300
    pinned = cases["pinned_gqa2_causal_113x257_d64"]["sink"]
    assert np.isneginf(pinned[0]) and list(pinned[1:]) == [-30.0, 0.0, 30.0]
    for n, c in cases.items():
        assert c["err_pt_bf16"].shape == c["err_pt_fp16"].shape == (5,) and (c["err_pt_bf16"] > 0).all(), n
        s = torch.from_numpy(c["sink"])
        assert torch.equal(s.bfloat16().float(), s) and torch.equal(s.half().float(), s), n      # exact in every sink dtype
        # rows without a key hold the sink in lse, zeros in out
        m = metas[n]
        for (sq_, sk_) in sr.sequences(c):
            vis = sr.visible(sq_.stop - sq_.start, sk_.stop - sk_.start, m["causal"], m["window"])
            empty = ~vis.any(-1)
            if empty.any():
                out = torch.from_numpy(c["out"]).reshape(-1, m["H"], m["D"])[sq_][empty]
                lse = torch.from_numpy(c["lse"]) if m["packed"] else torch.from_numpy(c["lse"]).transpose(0, 1).reshape(m["H"], -1)
                assert (out == 0).all() and torch.equal(lse[:, sq_][:, empty], s[:, None].expand(-1, int(empty.sum()))), n


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_standin_keeps_to_half_of_every_allowance(cases, dtype):
    """A condition on the FIXTURE (seeds and shapes were chosen for it), not a tolerance on the kernels: the kernels' roundings alone -- out rounded, scaled and
    rounded again, P and dS rounded -- use at most half of what the reference's rules allow, which leaves the GPU's summation order the other half.  dsink, one
    noisy sum per head, is held to that on sixteen realisations of the forward's rounding noise (tests/_sink_ref.py standin), the rest on three."""
    for name, case in cases.items():
        for variant in sr.DSINK_VARIANTS:
            res = sr.compare(case, sr.standin(case, dtype, variant=variant), dtype)
            assert res["dsink"] <= 0.5, (name, variant, res)
            if variant in sr.STANDIN_VARIANTS:
                assert all(res[q] <= 0.5 for q in sr.QUANTITIES), (name, variant, res)
                assert res["lse"] < sr.LSE_TOL / 2, (name, variant, res)


@pytest.mark.parametrize("mistake", sr.MISTAKES)
def test_the_comparison_reports_a_planted_mistake(cases, mistake):
    caught = []
    for name, case in cases.items():
        res = sr.compare(case, sr.standin(case, torch.bfloat16, mistake), torch.bfloat16)
        if any(res[q] > 1.0 for q in sr.QUANTITIES) or not res["lse"] < sr.LSE_TOL:
            caught.append(name)
    assert caught, mistake
    if mistake == "dsink_sign":
        assert len(caught) == len(cases), (mistake, caught)                                  # wrong everywhere
    if mistake == "lse_without_sink":                                                          # (a sink far below a row's lse changes little: not every case shows it)
        assert len(caught) >= 8 and "pinned_gqa2_causal_113x257_d64" in caught, (mistake, caught)
    if mistake in ("empty_lse_inf", "empty_rows_in_dsink"):                                    # ... exactly where rows without a key exist
        assert sorted(caught) == ["mqa8_causal_140x77_d64", "pinned_mqa4_causal_140x77_d64", "pk_mqa2_window31_d128"], (mistake, caught)
    if mistake == "sink_per_kv_head":
        assert "mha_full_64x300_d128" not in caught and "mha_causal_113x113_d256" not in caught and len(caught) >= 8, caught


def test_kernels_use_no_scratch(lib, monkeypatch):
    """No private segment, no spills; and the library holds the three kernels the design names."""
    from tests import _kernel_census as kc
    monkeypatch.setattr(kc, "LIB", cs.library_path())
    meta = kc.kernel_metadata()
    assert sorted(re.match(r"_ZN2fs\d+(fa_sink_\w+?_kernel)", n).group(1) for n in meta) == ["fa_sink_apply_kernel", "fa_sink_dsink_finish_kernel",
                                                                                             "fa_sink_dsink_partial_kernel"], list(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)          # two workgroups of 256 threads per SIMD at least
