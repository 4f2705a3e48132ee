"""ctypes binding of the C ABI in include/fa_gfx950_combine.h (libfa_gfx950_combine.so).

The structs mirror ``FaCombineSource`` / ``FaCombineParams`` field for field; ``load()`` checks the library's ``fa_sizeof_*`` and
``fa_combine_abi_version()`` against this file.  The library is opened on first use, not when the package is imported: everything else works
with libfa_gfx950.so alone.  There is no fallback: without the library ``load()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os

FA_COMBINE_ABI_VERSION = 1
FA_COMBINE_MAX_SOURCES = 2
FA_COMBINE_MAX_SPLITS = 256
FA_COMBINE_ROWS_MAX_SPLITS = 8
FA_COMBINE_DTYPE_FP16, FA_COMBINE_DTYPE_BF16, FA_COMBINE_DTYPE_FP32 = 0, 1, 3
FA_COMBINE_PATH_AUTO, FA_COMBINE_PATH_ROWS, FA_COMBINE_PATH_SPLITS = 0, 1, 2
FA_OK, FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_ERR_LAUNCH = 0, -1, -2, -3

_i64, _i32, _vp = C.c_int64, C.c_int32, C.c_void_p


class FaCombineSource(C.Structure):
    _fields_ = [
        ("o", _vp), ("lse", _vp),
        ("o_split_stride", _i64), ("o_batch_stride", _i64), ("o_row_stride", _i64), ("o_head_stride", _i64),
        ("lse_split_stride", _i64), ("lse_batch_stride", _i64), ("lse_row_stride", _i64), ("lse_head_stride", _i64),
        ("n_splits", _i32), ("dtype", _i32),
    ]


class FaCombineParams(C.Structure):
    _fields_ = [
        ("src", FaCombineSource * FA_COMBINE_MAX_SOURCES),
        ("out", _vp), ("lse", _vp),
        ("out_batch_stride", _i64), ("out_row_stride", _i64), ("out_head_stride", _i64),
        ("lse_batch_stride", _i64), ("lse_row_stride", _i64), ("lse_head_stride", _i64),
        ("n_sources", _i32), ("out_dtype", _i32), ("b", _i32), ("s", _i32), ("h", _i32), ("d", _i32),
        ("empty_lse_sign", _i32), ("path", _i32),
    ]


EXPORTS = (
    "fa_combine_abi_version", "fa_sizeof_combine_source", "fa_sizeof_combine_params", "fa_combine_last_error", "fa_combine_last_kernel_name",
    "fa_combine",
)

_LIB = None


def library_path() -> str:
    env = os.environ.get("FA_GFX950_COMBINE_LIB")
    if env:
        return env
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libfa_gfx950_combine.so")


def load():
    """dlopen libfa_gfx950_combine.so and type its entry points (raises if absent or mismatched)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `python flash-attention_amd/build.py` "
            "(the merge of partial attention results has no CPU or PyTorch fallback)")
    lib = C.CDLL(path)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise ImportError(f"{path} does not export {name}")
    for fn in (lib.fa_combine_abi_version, lib.fa_sizeof_combine_source, lib.fa_sizeof_combine_params):
        fn.argtypes = []
        fn.restype = C.c_int
    lib.fa_combine_last_error.restype = C.c_char_p
    lib.fa_combine_last_kernel_name.restype = C.c_char_p
    lib.fa_combine.argtypes = [C.POINTER(FaCombineParams), C.c_void_p]
    lib.fa_combine.restype = C.c_int
    if lib.fa_combine_abi_version() != FA_COMBINE_ABI_VERSION:
        raise ImportError(f"{path}: ABI version {lib.fa_combine_abi_version()} != binder {FA_COMBINE_ABI_VERSION}")
    if lib.fa_sizeof_combine_source() != C.sizeof(FaCombineSource) or lib.fa_sizeof_combine_params() != C.sizeof(FaCombineParams):
        raise ImportError(f"{path}: parameter-block size mismatch with the ctypes mirror")
    _LIB = lib
    return lib


def check(rc: int) -> None:
    """A negative return code becomes a RuntimeError carrying the library's message."""
    if rc != FA_OK:
        msg = load().fa_combine_last_error().decode("utf-8", "replace")
        raise RuntimeError(msg or f"libfa_gfx950_combine error {rc}")


def last_kernel_name() -> str:
    return load().fa_combine_last_kernel_name().decode()
