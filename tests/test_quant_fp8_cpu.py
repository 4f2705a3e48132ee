"""libfa_gfx950_quant.so without a GPU: the header, the ctypes mirror and the built library agree; every rule of the layout contract is answered with its
error code and a message before anything touches a device (the pointers here are made-up addresses: a call that got past validation would fault); the
library is opened on first use only; and the CPU reference the GPU tests compare against has the error bound three mantissa bits allow."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._quant_ref import dequant, quant_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "flash-attention_amd")
BASE = 0x7F0000000000          # a 16-byte aligned address that is never dereferenced
B, S, H, HK, D = 2, 5, 4, 2, 64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "libfa_gfx950_quant.so")):
        subprocess.check_call([sys.executable, os.path.join(PKG, "build.py")])
    from flash_attn_amd import _cabi_quant
    return _cabi_quant.load()


def _declared_functions():
    hdr = open(os.path.join(ROOT, "include", "fa_gfx950_quant.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(fa_[a-z_0-9]+)\s*\(", hdr)))


def _params(n=3, path=1, static=False, heads=H, rows=S, d=D, workspace=True):
    """A valid call on dense (B, rows, heads, d) tensors at made-up addresses."""
    from flash_attn_amd import _cabi_quant as q
    a = q.FaQuantParams()
    a.n_tensors, a.b, a.h_k, a.d, a.dtype, a.path = n, B, HK, d, 1, path
    for i in range(min(n, 3)):
        t = a.t[i]
        t.x, t.y, t.descale = BASE + (i << 32), BASE + (i << 32) + (1 << 28), BASE + (i << 32) + (1 << 29)
        t.x_batch_stride, t.x_row_stride, t.x_head_stride = rows * heads * d, heads * d, d
        t.y_batch_stride, t.y_row_stride, t.y_head_stride = rows * heads * d, heads * d, d
        t.descale_batch_stride, t.descale_head_stride = HK, 1
        t.heads, t.rows, t.is_static = heads, rows, int(static)
    if workspace:
        a.workspace, a.workspace_bytes = BASE + (7 << 32), 1 << 20
    return a


def _refused(lib, a, code, *words, sized=False):
    rc = lib.fa_quant_e4m3(C.byref(a), None)
    msg = lib.fa_quant_last_error().decode()
    assert rc == code, (rc, msg)
    assert msg.startswith("fa_quant_e4m3:") and all(w in msg for w in words), msg
    assert sized or lib.fa_quant_workspace_bytes(C.byref(a)) == 0          # (the workspace's own rules aside, the sizing query refuses the same calls)


def test_header_mirror_and_library_agree(lib):
    from flash_attn_amd import _cabi_quant as q
    names = _declared_functions()
    assert set(names) == set(q.EXPORTS), (names, q.EXPORTS)
    raw = C.CDLL(q.library_path())
    for n in names:
        assert hasattr(raw, n), n
    assert lib.fa_quant_abi_version() == q.FA_QUANT_ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "fa_gfx950_quant.h")).read()
    assert int(re.search(r"#define FA_QUANT_ABI_VERSION (\d+)", hdr).group(1)) == q.FA_QUANT_ABI_VERSION
    assert int(re.search(r"#define FA_QUANT_ONE_LAUNCH_MAX_ELEMS (\d+)", hdr).group(1)) == q.FA_QUANT_ONE_LAUNCH_MAX_ELEMS
    assert lib.fa_sizeof_quant_tensor() == C.sizeof(q.FaQuantTensor)
    assert lib.fa_sizeof_quant_params() == C.sizeof(q.FaQuantParams)
    assert lib.fa_sizeof_quant_append_params() == C.sizeof(q.FaQuantAppendParams)


def test_ctypes_mirror_matches_c_structs(lib, tmp_path):
    """Field by field: a C program prints offsetof() of every member of the three structs."""
    from flash_attn_amd import _cabi_quant as q
    lines = []
    for cls in (q.FaQuantTensor, q.FaQuantParams, q.FaQuantAppendParams):
        for name, _ in cls._fields_:
            lines.append(f'  printf("{cls.__name__}.{name} %zu\\n", offsetof({cls.__name__}, {name}));')
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fa_gfx950_quant.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "offsets"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cls in (q.FaQuantTensor, q.FaQuantParams, q.FaQuantAppendParams):
        for name, _ in cls._fields_:
            assert int(got[f"{cls.__name__}.{name}"]) == getattr(cls, name).offset, (cls.__name__, name)


def test_a_valid_call_is_sized_without_a_device(lib):
    a = _params(path=1)
    assert lib.fa_quant_workspace_bytes(C.byref(a)) == 3 * B * HK * 4
    assert lib.fa_quant_workspace_bytes(C.byref(_params(path=0))) == 0          # 5 * 2 * 64 elements per group: one launch, no scratch
    assert lib.fa_quant_workspace_bytes(C.byref(_params(path=1, static=True))) == 0
    a = _params(path=1)
    a.t[1].is_static = 1
    assert lib.fa_quant_workspace_bytes(C.byref(a)) == 2 * B * HK * 4
    assert lib.fa_quant_workspace_bytes(C.byref(_params(path=0, rows=1000))) == 3 * B * HK * 4   # 1000 * 2 * 64 > 16384: two passes


@pytest.mark.parametrize("slot", [0, 1, 2])
def test_each_layout_rule_is_refused_per_tensor_slot(lib, slot):
    name = f"tensor {slot}"
    for field in ("x", "y"):
        a = _params()
        setattr(a.t[slot], field, getattr(a.t[slot], field) + 8)                  # pointer 8 bytes off
        _refused(lib, a, -1, name, field, "16-byte aligned")
    a = _params()
    a.t[slot].x_row_stride = H * D + 1                                             # odd input row stride
    _refused(lib, a, -1, name, "x row stride", "multiple of 8 elements")
    a = _params()
    a.t[slot].x_head_stride = D + 4
    _refused(lib, a, -1, name, "x head stride", "multiple of 8 elements")
    a = _params()
    a.t[slot].y_head_stride = D + 4                                                # output head stride D + 4
    _refused(lib, a, -1, name, "y head stride", "multiple of 16 bytes")
    for which in ("batch", "row", "head"):
        a = _params()
        setattr(a.t[slot], f"y_{which}_stride", 0)                                 # zero output stride
        _refused(lib, a, -1, name, f"y {which} stride", "must not be 0")
    a = _params()
    a.t[slot].descale_head_stride = 0                                              # a dynamic descale is an output too
    _refused(lib, a, -1, name, "descale head stride", "must not be 0")
    a = _params()
    a.t[slot].heads = 3                                                            # heads % Hk != 0
    _refused(lib, a, -1, name, "heads (3)", "multiple of h_k (2)")
    a = _params(path=2)
    a.t[slot].rows = 1000                                                          # forced one-launch on an oversized group
    _refused(lib, a, -1, name, "128000 elements", "16384")
    a = _params(path=2)
    a.t[slot].cu_seqlens = BASE + (5 << 32)
    _refused(lib, a, -1, name, "packed", "two-pass")
    a = _params()
    a.t[slot].x = None
    _refused(lib, a, -1, name, "non-NULL")


def test_call_wide_rules_are_refused(lib):
    _refused(lib, _params(d=40), -1, "head dimension", "multiple of 16", "40")     # D = 40
    _refused(lib, _params(n=4), -1, "n_tensors = 4", "1 to 3")                      # more than 3 tensors
    _refused(lib, _params(n=0), -1, "n_tensors = 0")
    _refused(lib, _params(path=3), -1, "path")
    a = _params()
    a.dtype = 2
    _refused(lib, a, -1, "fp16 or bf16")
    a = _params(workspace=False)                                                    # missing workspace
    _refused(lib, a, -4, "workspace missing or too small", "48 bytes", sized=True)
    a = _params()
    a.workspace_bytes = 47
    _refused(lib, a, -4, "workspace missing or too small", sized=True)
    a = _params()
    a.workspace += 2
    _refused(lib, a, -1, "workspace", "4-byte aligned", sized=True)


def test_any_stride_is_accepted_in_a_size_one_dimension(lib):
    from flash_attn_amd import _cabi_quant as q
    a = q.FaQuantParams()                                                           # b = 1, one row, one head: no stride is ever used
    a.n_tensors, a.b, a.h_k, a.d, a.dtype, a.path = 1, 1, 1, D, 1, 1
    t = a.t[0]
    t.x, t.y, t.descale, t.heads, t.rows = BASE, BASE + (1 << 28), BASE + (1 << 29), 1, 1
    t.x_batch_stride, t.x_row_stride, t.x_head_stride = 3, 5, 7
    t.y_batch_stride, t.y_row_stride, t.y_head_stride = 0, 1, 9
    t.descale_batch_stride, t.descale_head_stride = 0, 0
    assert lib.fa_quant_workspace_bytes(C.byref(a)) == 4, lib.fa_quant_last_error()
    t.rows, t.x_row_stride = 2, 5                                                   # ... and as soon as the dimension has two elements, its stride counts
    assert lib.fa_quant_workspace_bytes(C.byref(a)) == 0 and b"x row stride" in lib.fa_quant_last_error()


def _append_params():
    from flash_attn_amd import _cabi_quant as q
    a = q.FaQuantAppendParams()
    a.knew, a.vnew, a.kcache, a.vcache, a.k_descale, a.v_descale = (BASE + (i << 32) for i in range(6))
    for nm, rows in (("knew", 3), ("vnew", 3), ("kcache", 512), ("vcache", 512)):
        setattr(a, nm + "_batch_stride", rows * HK * D); setattr(a, nm + "_row_stride", HK * D); setattr(a, nm + "_head_stride", D)
    a.k_descale_batch_stride = a.v_descale_batch_stride = HK
    a.k_descale_head_stride = a.v_descale_head_stride = 1
    a.b, a.seqlen_new, a.h_k, a.d, a.dtype = B, 3, HK, D, 1
    return a


def test_append_rules_are_refused(lib):
    def refused(a, *words):
        rc = lib.fa_quant_kvcache_append(C.byref(a), None)
        msg = lib.fa_quant_last_error().decode()
        assert rc == -1 and msg.startswith("fa_quant_kvcache_append:") and all(w in msg for w in words), (rc, msg)

    for nm in ("knew", "vnew", "kcache", "vcache"):
        a = _append_params()
        setattr(a, nm, getattr(a, nm) + 8)
        refused(a, "16-byte aligned")
        a = _append_params()
        setattr(a, nm + "_row_stride", HK * D + 4)
        refused(a, nm, "row stride", "multiple of")
    a = _append_params()
    a.kcache_row_stride = 0
    refused(a, "kcache", "must not be 0")
    a = _append_params()
    a.d = 40
    refused(a, "multiple of 16")
    a = _append_params()
    a.dtype = 2
    refused(a, "fp16 or bf16")
    a = _append_params()
    a.k_descale = None
    refused(a, "non-NULL")
    a = _append_params()
    a.block_table, a.page_block_size = BASE + (9 << 32), 100
    refused(a, "divisible by 256")
    a.page_block_size, a.cache_batch_idx = 256, BASE + (10 << 32)
    refused(a, "cache_batch_idx")
    a = _append_params()
    a.seqlen_new = 0                                                                # nothing to append: accepted, nothing launched
    assert lib.fa_quant_kvcache_append(C.byref(a), None) == 0


def test_missing_quant_library_fails_on_first_use_only(tmp_path):
    code = ("import flash_attn_amd\n"
            "from flash_attn_amd import quantize_fp8, kvcache_append_fp8, _cabi, _cabi_quant\n"
            "_cabi.load()\n"
            "try:\n    _cabi_quant.load()\nexcept ImportError as e:\n    print('ImportError:', e)\n")
    env = dict(os.environ, FA_GFX950_QUANT_LIB=str(tmp_path / "absent.so"), PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ImportError:" in r.stdout and "absent.so not found" in r.stdout and "build.py" in r.stdout, r.stdout


def test_python_checks_refuse_before_the_library_is_needed():
    from flash_attn_amd import quantize_fp8
    with pytest.raises(RuntimeError, match="at least one"):
        quantize_fp8(num_heads_k=2)
    x = torch.zeros(1, 2, 2, 16, dtype=torch.bfloat16, requires_grad=True)
    with pytest.raises(RuntimeError, match="no backward"):
        quantize_fp8(x, num_heads_k=2)
    with pytest.raises(RuntimeError, match="CUDA device"):
        quantize_fp8(x.detach(), num_heads_k=2)


def test_reference_has_the_error_three_mantissa_bits_allow():
    """|x * inv - float(y)| <= max(2^-4 |x * inv|, 2^-10) (1 + 2^-20): half an ulp of a 3-bit mantissa (relative 2^-4), or half the smallest subnormal step
    (2^-9 / 2); the group maximum maps to +-448 exactly; and the reference's divisions are IEEE fp32 divisions."""
    g = torch.Generator().manual_seed(5)
    for dtype in (torch.bfloat16, torch.float16):
        x = (torch.randn(2, 37, 4, 64, generator=g) * 3).to(dtype)
        x[0, :, 0] *= 1e-3                                                          # one head far below its group's maximum: the subnormal range of e4m3
        y, ds = quant_ref(x, 2)
        assert not ((y.view(torch.uint8) & 0x7F) == 0x7F).any()
        amax = x.float().reshape(2, 37, 2, 128).abs().amax(dim=(1, 3))
        assert np.array_equal(ds.numpy(), amax.numpy() / np.float32(448)) and ds.dtype == torch.float32
        inv = (np.float32(1) / ds.numpy()).astype(np.float32)
        t = x.float().reshape(2, 37, 2, 128) * torch.from_numpy(inv)[:, None, :, None]
        err = (t - y.float().reshape(2, 37, 2, 128)).abs()
        assert bool((err <= torch.maximum(t.abs() * 2.0 ** -4, torch.tensor(2.0 ** -10)) * (1 + 2.0 ** -20)).all())
        assert torch.equal(y.float().reshape(2, 37, 2, 128).abs().amax(dim=(1, 3)), torch.full((2, 2), 448.0))
        assert torch.equal(dequant(y, ds), y.float() * ds.repeat_interleave(2, dim=1)[:, None, :, None])
    # static mode saturates, never NaN; an empty packed entry has descale 1
    x = torch.tensor([1000.0, -1000.0, 463.9, 464.0, 2.0 ** -10, 0.0] + [0.0] * 10).to(torch.bfloat16).reshape(1, 1, 1, 16)
    y, _ = quant_ref(x, 1, descale=torch.ones(1, 1))
    assert y.view(torch.uint8).flatten()[:6].tolist() == [0x7E, 0xFE, 0x7E, 0x7E, 0x00, 0x00]
    _, ds = quant_ref(torch.ones(3, 2, 16, dtype=torch.bfloat16), 2, cu_seqlens=[0, 0, 3])
    assert ds.tolist() == [[1.0, 1.0], [1.0 / 448, 1.0 / 448]] or torch.equal(ds, torch.tensor([[1.0, 1.0], [1 / 448, 1 / 448]], dtype=torch.float32))


def test_kernels_keep_their_tiles_in_registers(lib, monkeypatch):
    """The one-launch bound of the header is what a workgroup holds WITHOUT scratch: no kernel of the library has a private segment or spills, and the set of
    kernels is the eight the design names (clear, amax, and cast / one-launch / append for bf16 and fp16)."""
    from flash_attn_amd import _cabi_quant as q
    from tests import _kernel_census as kc
    monkeypatch.setattr(kc, "LIB", q.library_path())
    meta = kc.kernel_metadata()
    families = sorted(re.match(r"_ZN2fq\d+(fa_quant_\w+?_kernel)", n).group(1) + ("<bf16>" if "Lb1E" in n else "<fp16>" if "Lb0E" in n else "") for n in meta)
    assert families == ["fa_quant_amax_kernel", "fa_quant_append_kernel<bf16>", "fa_quant_append_kernel<fp16>", "fa_quant_cast_kernel<bf16>",
                        "fa_quant_cast_kernel<fp16>", "fa_quant_clear_kernel", "fa_quant_fused_kernel<bf16>", "fa_quant_fused_kernel<fp16>"], families
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)          # two workgroups of 256 threads per SIMD set at least
