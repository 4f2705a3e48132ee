"""ctypes binding of the C ABI in include/fa_gfx950_quant.h (libfa_gfx950_quant.so).

The structs mirror ``FaQuantTensor`` / ``FaQuantParams`` / ``FaQuantAppendParams`` field for field; ``load()`` checks the library's
``fa_sizeof_*`` and ``fa_quant_abi_version()`` against this file.  The library is opened on first use, not when the package is imported:
everything else works with libfa_gfx950.so alone.  There is no fallback: without the library ``load()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os

FA_QUANT_ABI_VERSION = 1
FA_QUANT_MAX_TENSORS = 3
FA_QUANT_ONE_LAUNCH_MAX_ELEMS = 16384
FA_QUANT_PATH_AUTO, FA_QUANT_PATH_TWO_PASS, FA_QUANT_PATH_ONE_LAUNCH = 0, 1, 2
FA_OK, FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_ERR_LAUNCH, FA_ERR_WORKSPACE = 0, -1, -2, -3, -4

_i64, _i32, _vp = C.c_int64, C.c_int32, C.c_void_p


class FaQuantTensor(C.Structure):
    _fields_ = [
        ("x", _vp), ("y", _vp), ("descale", _vp), ("cu_seqlens", _vp),
        ("x_batch_stride", _i64), ("x_row_stride", _i64), ("x_head_stride", _i64),
        ("y_batch_stride", _i64), ("y_row_stride", _i64), ("y_head_stride", _i64),
        ("descale_batch_stride", _i64), ("descale_head_stride", _i64),
        ("heads", _i32), ("rows", _i32), ("is_static", _i32), ("reserved", _i32),
    ]


class FaQuantParams(C.Structure):
    _fields_ = [
        ("t", FaQuantTensor * FA_QUANT_MAX_TENSORS),
        ("workspace", _vp), ("workspace_bytes", _i64),
        ("n_tensors", _i32), ("b", _i32), ("h_k", _i32), ("d", _i32), ("dtype", _i32), ("path", _i32), ("reserved", _i32 * 2),
    ]


class FaQuantAppendParams(C.Structure):
    _fields_ = [
        ("knew", _vp), ("vnew", _vp), ("kcache", _vp), ("vcache", _vp), ("k_descale", _vp), ("v_descale", _vp),
        ("knew_batch_stride", _i64), ("knew_row_stride", _i64), ("knew_head_stride", _i64),
        ("vnew_batch_stride", _i64), ("vnew_row_stride", _i64), ("vnew_head_stride", _i64),
        ("kcache_batch_stride", _i64), ("kcache_row_stride", _i64), ("kcache_head_stride", _i64),
        ("vcache_batch_stride", _i64), ("vcache_row_stride", _i64), ("vcache_head_stride", _i64),
        ("k_descale_batch_stride", _i64), ("k_descale_head_stride", _i64),
        ("v_descale_batch_stride", _i64), ("v_descale_head_stride", _i64),
        ("seqlens_k", _vp), ("cache_batch_idx", _vp), ("block_table", _vp), ("block_table_batch_stride", _i64),
        ("page_block_size", _i32), ("b", _i32), ("seqlen_new", _i32), ("h_k", _i32), ("d", _i32),
        ("dtype", _i32), ("reserved", _i32 * 2),
    ]


EXPORTS = (
    "fa_quant_abi_version", "fa_sizeof_quant_tensor", "fa_sizeof_quant_params", "fa_sizeof_quant_append_params", "fa_quant_last_error",
    "fa_quant_workspace_bytes", "fa_quant_e4m3", "fa_quant_kvcache_append",
)

_LIB = None


def library_path() -> str:
    env = os.environ.get("FA_GFX950_QUANT_LIB")
    if env:
        return env
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libfa_gfx950_quant.so")


def load():
    """dlopen libfa_gfx950_quant.so and type its entry points (raises if absent or mismatched)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `python flash-attention_amd/build.py` "
            "(the e4m3 quantisation has no CPU or PyTorch fallback)")
    lib = C.CDLL(path)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise ImportError(f"{path} does not export {name}")
    for fn in (lib.fa_quant_abi_version, lib.fa_sizeof_quant_tensor, lib.fa_sizeof_quant_params, lib.fa_sizeof_quant_append_params):
        fn.argtypes = []
        fn.restype = C.c_int
    lib.fa_quant_last_error.restype = C.c_char_p
    lib.fa_quant_workspace_bytes.argtypes = [C.POINTER(FaQuantParams)]
    lib.fa_quant_workspace_bytes.restype = C.c_int64
    lib.fa_quant_e4m3.argtypes = [C.POINTER(FaQuantParams), C.c_void_p]
    lib.fa_quant_e4m3.restype = C.c_int
    lib.fa_quant_kvcache_append.argtypes = [C.POINTER(FaQuantAppendParams), C.c_void_p]
    lib.fa_quant_kvcache_append.restype = C.c_int
    if lib.fa_quant_abi_version() != FA_QUANT_ABI_VERSION:
        raise ImportError(f"{path}: ABI version {lib.fa_quant_abi_version()} != binder {FA_QUANT_ABI_VERSION}")
    if (lib.fa_sizeof_quant_tensor() != C.sizeof(FaQuantTensor) or lib.fa_sizeof_quant_params() != C.sizeof(FaQuantParams)
            or lib.fa_sizeof_quant_append_params() != C.sizeof(FaQuantAppendParams)):
        raise ImportError(f"{path}: parameter-block size mismatch with the ctypes mirror")
    _LIB = lib
    return lib


def check(rc: int) -> None:
    """A negative return code becomes a RuntimeError carrying the library's message."""
    if rc != FA_OK:
        msg = load().fa_quant_last_error().decode("utf-8", "replace")
        raise RuntimeError(msg or f"libfa_gfx950_quant error {rc}")
