/*
 * fa_gfx950_quant.h -- C ABI of `libfa_gfx950_quant.so`: the producer side of the FP8 paths of libfa_gfx950.so (include/fa_gfx950.h).
 *
 * fa_fwd_fp8 / fa_varlen_fwd_fp8 / fa_fwd_kvcache_fp8 consume OCP e4m3 (float8_e4m3fn) tensors with one fp32 descale per (batch entry, KV head);
 * this library makes them from bf16 / fp16 activations on the GPU, and appends bf16 / fp16 keys / values to an e4m3 KV cache with the cache's scale.
 * It is a library of its own (own header, own version) so that the kernel set and the export list of libfa_gfx950.so stay what they are; the
 * error codes are the main header's (FA_OK 0, FA_ERR_INVALID_ARGUMENT -1, FA_ERR_UNSUPPORTED -2, FA_ERR_LAUNCH -3, FA_ERR_WORKSPACE -4).
 *
 * Semantics (exact: the tests compare bytes)
 *   A tensor has `heads` heads; r = heads / h_k.  The GROUP (b, g) is heads g*r .. g*r + r - 1 of batch entry b over all rows of that entry: `rows`
 *   rows of a fixed-length tensor (b, rows, heads, d), or rows cu_seqlens[b] .. cu_seqlens[b+1] - 1 of a packed one (rows = total, heads, d) -- the
 *   descale indexing of the consumers.
 *     dynamic:  amax = max |float(x)| over the group;  descale = amax > 0 ? amax / 448.0f : 1.0f  (a correctly rounded fp32 division; an empty group
 *               gives 1.0);  the descale is WRITTEN to descale[b * descale_batch_stride + g * descale_head_stride];
 *     static:   the descale is READ from there (the caller guarantees finite and > 0): a cache's scale;
 *     both:     inv = 1.0f / descale (correctly rounded);  y = e4m3_rne(min(max(float(x) * inv, -448), 448)).
 *   The clamp makes static mode saturate: 0x7F / 0xFF (NaN) never come from finite input.  Non-finite inputs, and groups so small that inv overflows
 *   (amax < 448 * 2^-128), are unspecified.
 *
 * Layout contract
 *   - x: 16-byte aligned, batch / row / head strides multiples of 8 ELEMENTS; a stride of 0 is accepted (an expanded input);
 *   - y: 16-byte aligned, strides multiples of 16 BYTES (= elements) and non-zero; a dynamic descale (an output) has non-zero strides too;
 *   - every rule applies to dimensions of more than one element only: the stride of a size-1 dimension is never used; the batch strides of a packed
 *     tensor are ignored;
 *   - d % 16 == 0, heads % h_k == 0, b * h_k <= 65535, and a group holds at most 2^30 16-element chunks;
 *   - the last (head-dim) stride is 1; all offsets are computed in 64 bits.
 *   A violation returns FA_ERR_INVALID_ARGUMENT with a message naming the entry point and the tensor slot before anything touches the device.
 *
 * No entry point synchronises with the host, reads device memory on the host or allocates: every call can be captured in a HIP graph.
 */
#ifndef FA_GFX950_QUANT_H_
#define FA_GFX950_QUANT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_QUANT_ABI_VERSION 1
#define FA_QUANT_MAX_TENSORS 3
/* The one-launch path keeps a whole group in the registers of one 256-thread workgroup: 4 chunks of 16 elements per thread = 32 VGPRs of payload, no
 * private segment.  A group of more elements (r * rows * d) takes the two-pass path. */
#define FA_QUANT_ONE_LAUNCH_MAX_ELEMS 16384

enum { FA_QUANT_PATH_AUTO = 0, FA_QUANT_PATH_TWO_PASS = 1, FA_QUANT_PATH_ONE_LAUNCH = 2 };

typedef struct FaQuantTensor {
  const void* x;                /* bf16 / fp16 (FaQuantParams::dtype): (b, rows, heads, d), or packed (rows = total, heads, d)   */
  void* y;                      /* e4m3, same shape, strides of its own                                                         */
  float* descale;               /* (b, h_k) fp32: written (dynamic) or read (static)                                            */
  const int32_t* cu_seqlens;    /* NULL => fixed-length; else device int32 (b + 1): the tensor is packed                         */
  int64_t x_batch_stride, x_row_stride, x_head_stride;   /* elements */
  int64_t y_batch_stride, y_row_stride, y_head_stride;   /* bytes    */
  int64_t descale_batch_stride, descale_head_stride;     /* elements */
  int32_t heads;
  int32_t rows;                 /* rows per batch entry; packed: total rows                                                      */
  int32_t is_static;            /* 0 = dynamic (descale is an output), 1 = static (descale is an input)                          */
  int32_t reserved;
} FaQuantTensor;

typedef struct FaQuantParams {
  FaQuantTensor t[FA_QUANT_MAX_TENSORS];   /* q, k and v of one step go into one call: all tensors share the launches            */
  void* workspace;              /* fa_quant_workspace_bytes() bytes, 4-byte aligned; may be NULL if that is 0.  Cleared by the call itself, in stream order */
  int64_t workspace_bytes;
  int32_t n_tensors;            /* 1 .. FA_QUANT_MAX_TENSORS                                                                     */
  int32_t b, h_k, d;
  int32_t dtype;                /* of every x: 0 = fp16, 1 = bf16 (FA_DTYPE_FP16 / FA_DTYPE_BF16 of the main header)              */
  int32_t path;                 /* FA_QUANT_PATH_*: 0 picks from the shapes -- one launch when every tensor is fixed-length and no group exceeds
                                   FA_QUANT_ONE_LAUNCH_MAX_ELEMS, else two passes (amax per group into the workspace, then the cast).  Forcing
                                   ONE_LAUNCH on a larger group or a packed tensor is FA_ERR_INVALID_ARGUMENT.  Both paths write identical bytes */
  int32_t reserved[2];
} FaQuantParams;

/* Quantising append: FaKvAppendParams of the main header with bf16 / fp16 knew / vnew (B, S_new, Hk, D; strides in elements), e4m3 caches (strides in
 * bytes) and the cache's scales: k_descale / v_descale (B, Hk), read at the batch entry of knew -- NOT at the cache row (fa_fwd_kvcache_fp8's
 * convention).  The bytes written equal static quantisation followed by fa_kvcache_append(dtype = FA_DTYPE_FP8_E4M3); K and V go in one launch. */
typedef struct FaQuantAppendParams {
  const void* knew;
  const void* vnew;
  void* kcache;
  void* vcache;
  const float* k_descale;
  const float* v_descale;
  int64_t knew_batch_stride, knew_row_stride, knew_head_stride;
  int64_t vnew_batch_stride, vnew_row_stride, vnew_head_stride;
  int64_t kcache_batch_stride, kcache_row_stride, kcache_head_stride;
  int64_t vcache_batch_stride, vcache_row_stride, vcache_head_stride;
  int64_t k_descale_batch_stride, k_descale_head_stride;
  int64_t v_descale_batch_stride, v_descale_head_stride;
  const int32_t* seqlens_k;         /* (B) current lengths; NULL => append at row 0 */
  const int32_t* cache_batch_idx;   /* optional                                      */
  const int32_t* block_table;       /* optional (paged cache, pages of a multiple of 256 rows) */
  int64_t block_table_batch_stride;
  int32_t page_block_size;
  int32_t b, seqlen_new, h_k, d;
  int32_t dtype;                    /* of knew / vnew: 0 = fp16, 1 = bf16 */
  int32_t reserved[2];
} FaQuantAppendParams;

int fa_quant_abi_version(void);
int fa_sizeof_quant_tensor(void);
int fa_sizeof_quant_params(void);
int fa_sizeof_quant_append_params(void);
/* Last error message of the calling thread ("" if none). */
const char* fa_quant_last_error(void);

/* Bytes of amax scratch fa_quant_e4m3 needs for these parameters (one 32-bit word per group of a dynamic tensor on the two-pass path; 0 on the
 * one-launch path, when every tensor is static, or when the parameters are invalid). */
int64_t fa_quant_workspace_bytes(const FaQuantParams* params);
/* Quantise up to three tensors.  Launches: one (one-launch path, or two-pass with static tensors only); a clear of the scratch, the amax kernel and
 * the cast kernel otherwise.  `stream` is a hipStream_t. */
int fa_quant_e4m3(const FaQuantParams* params, void* stream);
/* Quantise new keys / values with the cache's scales straight into the cache rows (contiguous, cache_batch_idx or paged): one launch. */
int fa_quant_kvcache_append(const FaQuantAppendParams* params, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA_GFX950_QUANT_H_ */
