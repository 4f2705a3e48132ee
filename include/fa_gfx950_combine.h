/*
 * fa_gfx950_combine.h -- C ABI of `libfa_gfx950_combine.so`: the merge of partial attention results.
 *
 * Every attention entry point of libfa_gfx950.so (include/fa_gfx950.h) returns (out, lse).  This library puts several such results over DISJOINT key
 * sets together: the chunks of a chunked-context prefill, a shared prefix and a per-request suffix, the steps of a ring, the splits of a split-KV
 * decode (FA3's flash_attn_combine).  It is a library of its own (own header, own version) so that the kernel set and the export list of
 * libfa_gfx950.so stay what they are; the error codes are the main header's (FA_OK 0, FA_ERR_INVALID_ARGUMENT -1, FA_ERR_UNSUPPORTED -2,
 * FA_ERR_LAUNCH -3).
 *
 * Operation, for every row (b, s, h) over the n partials (o_i, lse_i) of the call, in split order (source 0's splits, then source 1's):
 *     a partial is LIVE when lse_i is finite;  m = max of the live lse_i;
 *     lse = m + log(sum_live exp(lse_i - m));   out = sum_live (exp(lse_i - m) / sum) * o_i;
 *   natural log, fp32 arithmetic, one rounding to the output dtype at the end.
 *   - A partial whose lse is +inf or -inf is EMPTY (+inf is what this project's kernels return for a row without a visible key, -inf is FA3's marker).
 *     Its o row is NOT READ: NaN or garbage there never reaches the result.  A live partial whose weight underflows to 0 is not read either.
 *   - A row with no live partial gives out = 0 and lse = +inf (empty_lse_sign = +1) or -inf (empty_lse_sign = -1).
 *   - A NaN lse is unspecified.
 *   - The result depends on the values and the shapes only: it is bit-identical from run to run and between strided and contiguous tensors of the
 *     same values.  The rows kernel adds the partials in split order; the splits kernel gives split i to slot i % slots of its workgroup, adds each
 *     slot's partials in split order and then the slots in slot order.
 *   - A row with one live partial reproduces that partial: weight 1.0f and lse = m exactly.
 *
 * Sources.  A call takes one or two SOURCES, each a strided stack of n_splits partials with its own o dtype (fp16 / bf16 / fp32; lse is always fp32)
 * and its own strides: one source of S splits is FA3's combine, two sources of one split each the pairwise merge, a running fp32 accumulator plus
 * a stack of new partials 1 + S.  The splits of both sources total at most FA_COMBINE_MAX_SPLITS.
 * In place.  out / lse may be exactly source 0's tensors (same pointers, same strides) when source 0 has one split: every element is then read and
 * written by the same lane, and a row's lse is written after every lane of the row has read it.  Any other overlap is unspecified.
 *
 * Layout contract (the project's: include/fa_gfx950.h)
 *   - o pointers (sources and out): 16-byte aligned; the last (head-dim) stride is 1; every other stride, in bytes, is a multiple of 16 -- checked for
 *     dimensions of more than one element only: the stride of a size-1 dimension is never used;
 *   - a stride of 0 is accepted on a source (an expanded input) and refused on out / lse in a dimension of more than one element;
 *   - lse pointers: 4-byte aligned, any element strides ((B, H, S) tensors, (B, S, H) views and slices of them);
 *   - d % 8 == 0, 8 <= d <= 512;  b, s, h >= 0 with b * s * h < 2^31;  a call without rows returns FA_OK without a launch and without looking at
 *     pointers or strides;  every offset is computed in 64 bits.
 *   A violation returns FA_ERR_INVALID_ARGUMENT with a message naming the argument before anything touches the device.
 *
 * The call launches one kernel, does not synchronise with the host, reads no device memory on the host and allocates nothing: it can be captured in a
 * HIP graph.
 */
#ifndef FA_GFX950_COMBINE_H_
#define FA_GFX950_COMBINE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_COMBINE_ABI_VERSION 1
#define FA_COMBINE_MAX_SOURCES 2
#define FA_COMBINE_MAX_SPLITS 256
/* Path AUTO takes the splits kernel when the call has more than this many partials (or at least 4 and too few rows to fill the chip with the rows kernel). */
#define FA_COMBINE_ROWS_MAX_SPLITS 8

/* 0 and 1 are FA_DTYPE_FP16 / FA_DTYPE_BF16 of the main header; its 2 (e4m3) is not a dtype of this library. */
enum { FA_COMBINE_DTYPE_FP16 = 0, FA_COMBINE_DTYPE_BF16 = 1, FA_COMBINE_DTYPE_FP32 = 3 };
enum { FA_COMBINE_PATH_AUTO = 0, FA_COMBINE_PATH_ROWS = 1, FA_COMBINE_PATH_SPLITS = 2 };

typedef struct FaCombineSource {
  const void* o;                /* (n_splits, b, s, h, d) under the strides below, dtype `dtype`                         */
  const float* lse;             /* (n_splits, b, s, h) under the strides below                                           */
  int64_t o_split_stride, o_batch_stride, o_row_stride, o_head_stride;           /* elements */
  int64_t lse_split_stride, lse_batch_stride, lse_row_stride, lse_head_stride;   /* elements */
  int32_t n_splits;             /* >= 1                                                                                  */
  int32_t dtype;                /* FA_COMBINE_DTYPE_* of o                                                               */
} FaCombineSource;

typedef struct FaCombineParams {
  FaCombineSource src[FA_COMBINE_MAX_SOURCES];
  void* out;                    /* (b, s, h, d), dtype out_dtype                                                         */
  float* lse;                   /* (b, s, h) under its strides; may be NULL: the merged lse is not written               */
  int64_t out_batch_stride, out_row_stride, out_head_stride;   /* elements */
  int64_t lse_batch_stride, lse_row_stride, lse_head_stride;   /* elements */
  int32_t n_sources;            /* 1 .. FA_COMBINE_MAX_SOURCES                                                           */
  int32_t out_dtype;            /* FA_COMBINE_DTYPE_*                                                                    */
  int32_t b, s, h, d;           /* a packed (total, h, d) tensor is b = 1, s = total                                      */
  int32_t empty_lse_sign;       /* +1 or -1: the lse of a row with no live partial is +inf or -inf                       */
  int32_t path;                 /* FA_COMBINE_PATH_*: 0 picks from the shapes; both kernels take every valid call        */
} FaCombineParams;

int fa_combine_abi_version(void);
int fa_sizeof_combine_source(void);
int fa_sizeof_combine_params(void);
/* Last error message of the calling thread ("" if none). */
const char* fa_combine_last_error(void);
/* Name of the kernel the calling thread's last fa_combine launched ("" if it launched none: a refused call, a call without rows). */
const char* fa_combine_last_kernel_name(void);

/* Merge the partials: one launch.  `stream` is a hipStream_t. */
int fa_combine(const FaCombineParams* params, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA_GFX950_COMBINE_H_ */
