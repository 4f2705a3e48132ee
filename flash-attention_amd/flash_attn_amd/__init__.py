"""MI355X-native fused attention (gfx950 HIP kernels) behind the flash_attn Python interface."""
__version__ = "0.1.0"

from .flash_attn_interface import (  # noqa: F401
    flash_attn_func,
    flash_attn_kvpacked_func,
    flash_attn_padded_func,
    flash_attn_qkvpacked_func,
    flash_attn_varlen_func,
    flash_attn_varlen_kvpacked_func,
    flash_attn_varlen_qkvpacked_func,
    flash_attn_with_kvcache,
)
from .fp8_quant import kvcache_append_fp8, quantize_fp8  # noqa: F401
from .combine import flash_attn_combine, merge_attn_states  # noqa: F401
from .sink import (  # noqa: F401
    apply_attn_sink,
    flash_attn_sink_func,
    flash_attn_varlen_sink_func,
    flash_attn_with_kvcache_sink,
)
