"""CPU suite: the C-ABI library loads and exports every symbol include/fa_gfx950.h declares; the
ctypes mirror matches the C structs; the torch extension exposes the reference backend-module API;
argument validation raises before any GPU work.  (No compute calls without a GPU.)"""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "flash-attention_amd")


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(PKG, "libfa_gfx950.so")
    if not os.path.exists(lib):
        subprocess.check_call([sys.executable, os.path.join(PKG, "build.py")])
    return lib


def _declared_functions():
    hdr = open(os.path.join(ROOT, "include", "fa_gfx950.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(fa_[a-z_0-9]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol(built):
    from flash_attn_amd import _cabi
    names = _declared_functions()
    assert set(names) == set(_cabi.EXPORTS), (names, _cabi.EXPORTS)
    lib = ctypes.CDLL(built)
    for n in names:
        assert hasattr(lib, n), n


def test_ctypes_mirror_matches_c_structs(built):
    from flash_attn_amd import _cabi
    lib = _cabi.load()
    assert lib.fa_abi_version() == _cabi.FA_ABI_VERSION == 6
    assert lib.fa_sizeof_kvappend_params() == ctypes.sizeof(_cabi.FaKvAppendParams)
    assert lib.fa_sizeof_fwd_params() == ctypes.sizeof(_cabi.FaFwdParams)
    assert lib.fa_sizeof_bwd_params() == ctypes.sizeof(_cabi.FaBwdParams)


def test_cabi_rejects_bad_arguments_without_touching_the_gpu(built):
    from flash_attn_amd import _cabi
    lib = _cabi.load()
    a = _cabi.FaFwdParams()
    a.b, a.h, a.h_k, a.d, a.dtype = 1, 3, 2, 128, _cabi.FA_DTYPE_BF16
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT
    assert b"heads" in lib.fa_last_error()
    a.h_k, a.d = 1, 72   # the forward takes any multiple of 8 (run-time column bound): rejected later, for its NULL tensors
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"non-NULL" in lib.fa_last_error()
    a.d = 60
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"multiple of 8" in lib.fa_last_error()
    g = _cabi.FaBwdParams()   # the backward takes any multiple of 8 too (run-time column bound of the next built size's kernels)
    g.b, g.h, g.h_k, g.d, g.dtype = 1, 2, 1, 72, _cabi.FA_DTYPE_BF16
    assert lib.fa_bwd(ctypes.byref(g), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"non-NULL" in lib.fa_last_error()
    g.d = 260
    assert lib.fa_bwd(ctypes.byref(g), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"multiple of 8" in lib.fa_last_error()
    a.d, a.dtype = 128, 7
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT
    a.dtype = _cabi.FA_DTYPE_FP16
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT  # NULL tensors
    with pytest.raises(RuntimeError):
        _cabi.check(_cabi.FA_ERR_INVALID_ARGUMENT)


def test_cabi_contract_of_the_later_entry_points(built):
    """Dropout, KV-cache, rotary and workspace entry points: argument contract checked on the host, no launch."""
    from flash_attn_amd import _cabi
    lib = _cabi.load()
    assert lib.fa_sizeof_rotary_params() == ctypes.sizeof(_cabi.FaRotaryParams)
    dummy = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is rejected before a launch

    def fwd_params():
        a = _cabi.FaFwdParams()
        a.b, a.h, a.h_k, a.d, a.dtype = 2, 4, 2, 128, _cabi.FA_DTYPE_BF16
        a.q = a.k = a.v = a.o = a.softmax_lse = dummy
        a.seqlen_q, a.seqlen_k, a.total_q = 16, 512, 32
        return a

    a = fwd_params()
    a.p_dropout = 0.1                                   # dropout needs the device rng_state
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"rng_state" in lib.fa_last_error()
    a = fwd_params()
    a.p_dropout = 1.0
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"p_dropout" in lib.fa_last_error()
    a = fwd_params()
    a.randval = dummy                                   # return_softmax payload only with dropout
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"return_softmax" in lib.fa_last_error()
    a = fwd_params()
    a.num_splits = 4                                    # key splits belong to the KV-cache entry point
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"num_splits" in lib.fa_last_error()
    a = fwd_params()
    a.block_table = dummy                               # so do paged caches
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"fa_fwd_kvcache" in lib.fa_last_error()
    a = fwd_params()
    a.block_table, a.page_block_size = dummy, 100       # page size must be a multiple of 256 (flash_api.cpp:1318)
    assert lib.fa_fwd_kvcache(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"256" in lib.fa_last_error()
    a = fwd_params()
    a.block_table, a.page_block_size, a.leftpad_k, a.seqused_k = dummy, 256, dummy, dummy
    assert lib.fa_fwd_kvcache(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"leftpad_k" in lib.fa_last_error()
    a = fwd_params()
    a.p_dropout, a.rng_state = 0.1, dummy               # inference path: no dropout
    assert lib.fa_fwd_kvcache(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"inference" in lib.fa_last_error()
    # workspace sizing is pure host arithmetic: decode with idle CUs wants split-KV scratch, a full grid does not
    a = fwd_params()
    a.b, a.seqlen_q, a.seqlen_k, a.total_q = 1, 1, 32768, 1
    need = lib.fa_fwd_workspace_bytes(ctypes.byref(a))
    assert need > 0 and need % ((a.d + 1) * 4 * a.b * a.h * a.seqlen_q) == 0
    a.b = 512
    assert lib.fa_fwd_workspace_bytes(ctypes.byref(a)) == 0
    a.b, a.num_splits = 1, 8
    assert lib.fa_fwd_workspace_bytes(ctypes.byref(a)) == 8 * (a.d + 1) * 4 * a.h
    # varlen: a work list is requested only when the max_seqlen grid would be mostly empty
    a = fwd_params()
    a.cu_seqlens_q = a.cu_seqlens_k = dummy
    a.b, a.seqlen_q, a.seqlen_k, a.total_q = 160, 16384, 16384, 65536
    assert lib.fa_fwd_workspace_bytes(ctypes.byref(a)) > 0
    a.b, a.seqlen_q, a.seqlen_k = 16, 4096, 4096
    assert lib.fa_fwd_workspace_bytes(ctypes.byref(a)) == 0
    r = _cabi.FaRotaryParams()
    r.x = r.y = r.cos = r.sin = dummy
    r.b, r.s, r.h, r.d, r.rotary_dim, r.seqlen_ro, r.dtype = 1, 1, 1, 128, 24, 8, _cabi.FA_DTYPE_FP16
    assert lib.fa_rotary(ctypes.byref(r), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"divisible by 16" in lib.fa_last_error()
    r.rotary_dim = 256
    assert lib.fa_rotary(ctypes.byref(r), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"headdim" in lib.fa_last_error()
    bw = _cabi.FaBwdParams()
    bw.b, bw.h, bw.h_k, bw.d, bw.dtype = 1, 2, 2, 64, _cabi.FA_DTYPE_BF16
    for f in ("dout", "q", "k", "v", "o", "softmax_lse", "dq", "dk", "dv", "softmax_d"):
        setattr(bw, f, dummy)
    bw.p_dropout = 0.2
    assert lib.fa_bwd(ctypes.byref(bw), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"rng_state" in lib.fa_last_error()
    assert lib.fa_set_rng_state(1, 2, None, None) == _cabi.FA_ERR_INVALID_ARGUMENT


def _layout_entry_points():
    """name -> (fresh valid params, call, tensors as (pointer field, stride prefix)): the 16-bit entry points the layout contract of fa_gfx950.h covers.  Pointers are
    never dereferenced: every call is refused on the host, or passes the check and is refused further down for something else."""
    from flash_attn_amd import _cabi
    lib = _cabi.load()
    base = 0x10000
    D = 64

    def strides(p, names, h, rows):
        for n in names:
            setattr(p, n + "_batch_stride", rows * h * D); setattr(p, n + "_row_stride", h * D); setattr(p, n + "_head_stride", D)

    def fwd(varlen=False, kvcache=False):
        a = _cabi.FaFwdParams()
        a.b, a.h, a.h_k, a.d, a.dtype = 2, 4, 2, D, _cabi.FA_DTYPE_BF16
        a.q, a.k, a.v, a.o, a.softmax_lse = (ctypes.c_void_p(base * i) for i in (1, 2, 3, 4, 5))
        a.seqlen_q, a.seqlen_k, a.total_q = 16, 512, 32
        strides(a, ("q", "o"), 4, 16); strides(a, ("k", "v"), 2, 512)
        if varlen:
            a.cu_seqlens_q = a.cu_seqlens_k = ctypes.c_void_p(base * 6)
        return a

    def bwd(varlen=False):
        g = _cabi.FaBwdParams()
        g.b, g.h, g.h_k, g.d, g.dtype = 2, 4, 2, D, _cabi.FA_DTYPE_BF16
        for i, f in enumerate(("dout", "q", "k", "v", "o", "softmax_lse", "dq", "dk", "dv", "softmax_d")):
            setattr(g, f, ctypes.c_void_p(base * (i + 1)))
        g.seqlen_q, g.seqlen_k, g.total_q, g.total_k = 16, 512, 32, 1024
        strides(g, ("do", "q", "o", "dq"), 4, 16); strides(g, ("k", "v", "dk", "dv"), 2, 512)
        if varlen:
            g.cu_seqlens_q = g.cu_seqlens_k = ctypes.c_void_p(base * 11)
        return g

    def append():
        p = _cabi.FaKvAppendParams()
        p.knew, p.vnew, p.kcache, p.vcache = (ctypes.c_void_p(base * i) for i in (1, 2, 3, 4))
        p.b, p.seqlen_new, p.h_k, p.d, p.dtype = 2, 16, 2, D, _cabi.FA_DTYPE_BF16
        strides(p, ("knew", "vnew"), 2, 16); strides(p, ("kcache", "vcache"), 2, 512)
        return p

    def rotary():
        r = _cabi.FaRotaryParams()
        r.x, r.y, r.cos, r.sin = (ctypes.c_void_p(base * i) for i in (1, 2, 3, 4))
        r.b, r.s, r.h, r.d, r.rotary_dim, r.seqlen_ro, r.dtype = 2, 16, 4, D, 32, 64, _cabi.FA_DTYPE_BF16
        strides(r, ("x", "y"), 4, 16)
        return r

    QO, KV = (("q", "q"), ("o", "o")), (("k", "k"), ("v", "v"))
    G = (("dout", "do"), ("q", "q"), ("o", "o"), ("dq", "dq"), ("k", "k"), ("v", "v"), ("dk", "dk"), ("dv", "dv"))
    return {
        "fa_fwd": (fwd, lambda a: lib.fa_fwd(ctypes.byref(a), None), QO + KV),
        "fa_varlen_fwd": (lambda: fwd(varlen=True), lambda a: lib.fa_varlen_fwd(ctypes.byref(a), None), QO + KV),
        "fa_fwd_kvcache": (fwd, lambda a: lib.fa_fwd_kvcache(ctypes.byref(a), None), QO + KV),
        "fa_bwd": (bwd, lambda g: lib.fa_bwd(ctypes.byref(g), None), G),
        "fa_varlen_bwd": (lambda: bwd(varlen=True), lambda g: lib.fa_varlen_bwd(ctypes.byref(g), None), G),
        "fa_kvcache_append": (append, lambda p: lib.fa_kvcache_append(ctypes.byref(p), None), (("knew", "knew"), ("vnew", "vnew"), ("kcache", "kcache"), ("vcache", "vcache"))),
        "fa_rotary": (rotary, lambda r: lib.fa_rotary(ctypes.byref(r), None), (("x", "x"), ("y", "y"))),
        "fa_fwd_schedule_query": (fwd, lambda a: min(lib.fa_fwd_schedule_query(ctypes.byref(a), 0), 0), QO + KV),
        "fa_bwd_dq_schedule_query": (bwd, lambda g: min(lib.fa_bwd_dq_schedule_query(ctypes.byref(g)), 0), G),
        "fa_bwd_plan_query": (bwd, lambda g: min(lib.fa_bwd_plan_query(ctypes.byref(g), (ctypes.c_int32 * 8)(), 8), 0), G),
    }


_LAYOUT_ENTRY_POINTS = ("fa_fwd", "fa_varlen_fwd", "fa_fwd_kvcache", "fa_bwd", "fa_varlen_bwd", "fa_kvcache_append", "fa_rotary", "fa_fwd_schedule_query",
                        "fa_bwd_dq_schedule_query", "fa_bwd_plan_query")


@pytest.mark.parametrize("entry", _LAYOUT_ENTRY_POINTS)
def test_cabi_layout_contract_of_the_16bit_entry_points(built, entry):
    """Pointers 16-byte aligned, strides of dimensions with more than one element multiples of 8 elements, outputs with non-zero strides (include/fa_gfx950.h): a
    violation is FA_ERR_INVALID_ARGUMENT naming the entry point and the tensor, on a NULL stream, before anything could touch the device."""
    from flash_attn_amd import _cabi
    lib = _cabi.load()
    make, call, tensors = _layout_entry_points()[entry]
    packed = "varlen" in entry
    outputs = set() if "query" in entry else {"dq", "dk", "dv"} if "bwd" in entry else {"o", "kcache", "vcache", "y"}   # (the queries write nothing)

    def refused(p, tensor):
        msg = lib.fa_last_error().decode() if call(p) == _cabi.FA_ERR_INVALID_ARGUMENT else None
        return msg is not None and entry in msg and (" " + tensor + " ") in msg.replace(",", " ").replace(":", " ") and ("16-byte" in msg or "stride" in msg)

    for ptr, st in tensors:
        p = make()
        setattr(p, ptr, ctypes.c_void_p(getattr(p, ptr) + 8))   # a base pointer off by 8 bytes
        assert refused(p, ptr), (entry, ptr, "pointer + 8", lib.fa_last_error())
        p = make()
        setattr(p, st + "_row_stride", getattr(p, st + "_row_stride") + 1)   # an odd row stride
        assert refused(p, ptr), (entry, ptr, "odd row stride", lib.fa_last_error())
        p = make()
        setattr(p, st + "_head_stride", 64 + 4)   # heads D + 4 apart
        assert refused(p, ptr), (entry, ptr, "head stride D + 4", lib.fa_last_error())
        if not packed:
            p = make()
            setattr(p, st + "_batch_stride", getattr(p, st + "_batch_stride") + 4)
            assert refused(p, ptr), (entry, ptr, "batch stride + 4", lib.fa_last_error())
        p = make()
        setattr(p, st + "_head_stride", 0)   # stride 0: an expanded input is accepted, an output is not
        if ptr in outputs:
            assert refused(p, ptr) and b"non-zero" in lib.fa_last_error(), (entry, ptr)


def test_cabi_layout_contract_ignores_the_stride_of_a_dimension_of_one(built):
    """torch gives a dimension of one element an arbitrary stride (one KV head, B = 1, one query row): neither refused nor used -- the schedule
    and sizing queries, which run the same check as the launching calls, answer as they do for even strides (nothing is launched here: the pointers are dummies)."""
    from flash_attn_amd import _cabi
    lib = _cabi.load()
    make, _, _ = _layout_entry_points()["fa_fwd"]
    a = make()
    a.b, a.h_k, a.seqlen_q, a.total_q = 1, 1, 1, 1
    want = lib.fa_fwd_schedule_query(ctypes.byref(a), 0)
    ws = lib.fa_fwd_workspace_bytes(ctypes.byref(a))
    a.q_batch_stride, a.o_batch_stride = 7, 0   # (not k / v: the workspace query is the KV-cache path's, where the cache's batch extent is not a parameter)
    a.k_head_stride, a.v_head_stride, a.q_row_stride, a.o_row_stride = 3, 5, 9, 0
    assert want > 0 and lib.fa_fwd_schedule_query(ctypes.byref(a), 0) == want
    assert ws > 0 and lib.fa_fwd_workspace_bytes(ctypes.byref(a)) == ws
    a.q_head_stride = 68   # ... while the four query heads are stepped
    assert lib.fa_fwd_schedule_query(ctypes.byref(a), 0) == _cabi.FA_ERR_INVALID_ARGUMENT and b"head stride of q" in lib.fa_last_error()
    assert lib.fa_fwd_workspace_bytes(ctypes.byref(a)) == 0
    # the launching call itself: with no query row there is nothing to write, and fa_fwd returns FA_OK right after the layout check without enqueuing anything
    a.seqlen_q = a.total_q = 0
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"fa_fwd: the head stride of q" in lib.fa_last_error()
    a.q_head_stride = 64
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_OK
    a.b, a.q_batch_stride, a.o_batch_stride = 2, 8, 0   # two batch entries: now the output's batch stride is stepped
    assert lib.fa_fwd(ctypes.byref(a), None) == _cabi.FA_ERR_INVALID_ARGUMENT and b"batch stride of the output o must be non-zero" in lib.fa_last_error()
    make, _, _ = _layout_entry_points()["fa_bwd"]
    g = make()
    g.b, g.h_k = 1, 1
    plan = (ctypes.c_int32 * 8)()
    want = lib.fa_bwd_dq_schedule_query(ctypes.byref(g))
    for t in ("do", "q", "k", "v", "o", "dq", "dk", "dv"):
        setattr(g, t + "_batch_stride", 3)
    g.k_head_stride, g.v_head_stride, g.dk_head_stride, g.dv_head_stride = 1, 3, 0, 7
    assert want > 0 and lib.fa_bwd_dq_schedule_query(ctypes.byref(g)) == want and lib.fa_bwd_plan_query(ctypes.byref(g), plan, 8) == 8
    g.dk_row_stride = 12
    assert lib.fa_bwd_dq_schedule_query(ctypes.byref(g)) == _cabi.FA_ERR_INVALID_ARGUMENT and b"row stride of dk" in lib.fa_last_error()


def test_torch_extension_is_the_reference_backend_module(built):
    import flash_attn_2_cuda as m
    for fn in ("fwd", "varlen_fwd", "bwd", "varlen_bwd", "fwd_kvcache"):
        assert callable(getattr(m, fn))
    q = torch.zeros(1, 4, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="CUDA"):
        m.fwd(q, q, q, None, None, 0.0, 0.125, False, -1, -1, 0.0, False, None)
    with pytest.raises(RuntimeError, match="generator"):
        m.fwd(q, q, q, None, None, 0.0, 0.125, False, -1, -1, 0.0, False, torch.Generator())
    with pytest.raises(RuntimeError, match="CUDA"):
        m.fwd_kvcache(q, q, q, None, None, None, None, None, None, None, None, None, None, 0.125, False, -1, -1, 0.0, True, 0)
    assert os.path.dirname(m.__file__) == PKG  # in-tree build, not site-packages


def test_ctypes_backend_validation_matches():
    from flash_attn_amd import backend as be
    q = torch.zeros(1, 4, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="CUDA"):
        be.fwd(q, q, q, None, None, 0.0, 0.125, False, -1, -1, 0.0, False, None)
    with pytest.raises(RuntimeError, match="generator"):
        be.fwd(q, q, q, None, None, 0.0, 0.125, False, -1, -1, 0.0, False, torch.Generator())
    with pytest.raises(RuntimeError, match="p_dropout"):
        be.fwd(q, q, q, None, None, 1.0, 0.125, False, -1, -1, 0.0, False, None)
    with pytest.raises(RuntimeError, match="CUDA"):  # dropout is built: the device check comes first
        be.fwd(q, q, q, None, None, 0.1, 0.125, False, -1, -1, 0.0, False, None)


def test_interface_mirror_exports_reference_names():
    import flash_attn_amd
    from flash_attn_amd import flash_attn_interface as fi
    for n in ("flash_attn_func", "flash_attn_varlen_func", "flash_attn_qkvpacked_func", "flash_attn_kvpacked_func",
              "flash_attn_varlen_qkvpacked_func", "flash_attn_varlen_kvpacked_func", "flash_attn_with_kvcache",
              "_flash_attn_forward", "_flash_attn_backward", "_flash_attn_varlen_forward", "_flash_attn_varlen_backward"):
        assert callable(getattr(fi, n))
    assert fi.flash_attn_gpu.__name__ in ("flash_attn_2_cuda", "flash_attn_amd.backend")


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from flash_attn_amd import _cabi
    monkeypatch.setattr(_cabi, "_LIB", None)
    monkeypatch.setenv("FA_GFX950_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError, match="no CPU or PyTorch fallback"):
        _cabi.load()
