"""ctypes binding of the C ABI in include/fa_gfx950_sink.h (libfa_gfx950_sink.so).

The structs mirror ``FaSinkApplyParams`` / ``FaSinkDsinkParams`` field for field; ``load()`` checks the library's ``fa_sink_sizeof_*`` and
``fa_sink_abi_version()`` against this file.  The library is opened on first use, not when the package is imported: everything else works
with libfa_gfx950.so alone.  There is no fallback: without the library ``load()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os

FA_SINK_ABI_VERSION = 1
FA_SINK_DSINK_MAX_BLOCKS = 64
FA_SINK_DTYPE_FP16, FA_SINK_DTYPE_BF16, FA_SINK_DTYPE_FP32 = 0, 1, 3
FA_OK, FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_ERR_LAUNCH = 0, -1, -2, -3

_i64, _i32, _vp = C.c_int64, C.c_int32, C.c_void_p


class FaSinkApplyParams(C.Structure):
    _fields_ = [
        ("out_in", _vp), ("lse_in", _vp), ("sink", _vp), ("out", _vp), ("lse", _vp), ("lse_bwd", _vp),
        ("out_in_batch_stride", _i64), ("out_in_row_stride", _i64), ("out_in_head_stride", _i64),
        ("lse_in_batch_stride", _i64), ("lse_in_row_stride", _i64), ("lse_in_head_stride", _i64),
        ("out_batch_stride", _i64), ("out_row_stride", _i64), ("out_head_stride", _i64),
        ("lse_batch_stride", _i64), ("lse_row_stride", _i64), ("lse_head_stride", _i64),
        ("lse_bwd_batch_stride", _i64), ("lse_bwd_row_stride", _i64), ("lse_bwd_head_stride", _i64),
        ("sink_stride", _i64),
        ("dtype", _i32), ("sink_dtype", _i32), ("b", _i32), ("s", _i32), ("h", _i32), ("d", _i32),
    ]


class FaSinkDsinkParams(C.Structure):
    _fields_ = [
        ("softmax_d", _vp), ("lse_bwd", _vp), ("sink", _vp), ("dsink", _vp), ("workspace", _vp),
        ("softmax_d_batch_stride", _i64), ("softmax_d_row_stride", _i64), ("softmax_d_head_stride", _i64),
        ("lse_bwd_batch_stride", _i64), ("lse_bwd_row_stride", _i64), ("lse_bwd_head_stride", _i64),
        ("sink_stride", _i64), ("dsink_stride", _i64),
        ("workspace_bytes", _i64),
        ("sink_dtype", _i32), ("b", _i32), ("s", _i32), ("h", _i32),
    ]


EXPORTS = (
    "fa_sink_abi_version", "fa_sink_sizeof_apply_params", "fa_sink_sizeof_dsink_params", "fa_sink_last_error", "fa_sink_last_kernel_name",
    "fa_sink_apply", "fa_sink_dsink_workspace_bytes", "fa_sink_dsink",
)

_LIB = None


def library_path() -> str:
    env = os.environ.get("FA_GFX950_SINK_LIB")
    if env:
        return env
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libfa_gfx950_sink.so")


def load():
    """dlopen libfa_gfx950_sink.so and type its entry points (raises if absent or mismatched)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `python flash-attention_amd/build.py` "
            "(attention sinks have no CPU or PyTorch fallback)")
    lib = C.CDLL(path)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise ImportError(f"{path} does not export {name}")
    for fn in (lib.fa_sink_abi_version, lib.fa_sink_sizeof_apply_params, lib.fa_sink_sizeof_dsink_params):
        fn.argtypes = []
        fn.restype = C.c_int
    lib.fa_sink_last_error.restype = C.c_char_p
    lib.fa_sink_last_kernel_name.restype = C.c_char_p
    lib.fa_sink_apply.argtypes = [C.POINTER(FaSinkApplyParams), C.c_void_p]
    lib.fa_sink_apply.restype = C.c_int
    lib.fa_sink_dsink_workspace_bytes.argtypes = [C.POINTER(FaSinkDsinkParams)]
    lib.fa_sink_dsink_workspace_bytes.restype = C.c_size_t
    lib.fa_sink_dsink.argtypes = [C.POINTER(FaSinkDsinkParams), C.c_void_p]
    lib.fa_sink_dsink.restype = C.c_int
    if lib.fa_sink_abi_version() != FA_SINK_ABI_VERSION:
        raise ImportError(f"{path}: ABI version {lib.fa_sink_abi_version()} != binder {FA_SINK_ABI_VERSION}")
    if lib.fa_sink_sizeof_apply_params() != C.sizeof(FaSinkApplyParams) or lib.fa_sink_sizeof_dsink_params() != C.sizeof(FaSinkDsinkParams):
        raise ImportError(f"{path}: parameter-block size mismatch with the ctypes mirror")
    _LIB = lib
    return lib


def check(rc: int) -> None:
    """A negative return code becomes a RuntimeError carrying the library's message."""
    if rc != FA_OK:
        msg = load().fa_sink_last_error().decode("utf-8", "replace")
        raise RuntimeError(msg or f"libfa_gfx950_sink error {rc}")


def last_kernel_name() -> str:
    return load().fa_sink_last_kernel_name().decode()
