/*
 * fa_gfx950_sink.h -- C ABI of `libfa_gfx950_sink.so`: learnable attention sinks as an exact post-pass.
 *
 * A sink is one learnable logit per QUERY head that joins the softmax denominator and carries no value row (gpt-oss style models).  It factors out
 * of the attention kernels exactly.  With (out, lse) what any entry point of libfa_gfx950.so (include/fa_gfx950.h) returns for a row and s the sink
 * of the row's head,
 *     lse' = log(exp(lse) + exp(s)),     out' = out / (1 + exp(s - lse)),
 * and the unchanged backward, given (out', lse'), recomputes the sinked probabilities P' = exp(S - lse') and returns softmax_d = rowsum(dO * out'),
 * from which
 *     dsink[h] = - sum over (b, row) of exp(s_h - lse'[b, h, row]) * softmax_d[b, h, row].
 * This is a library of its own (own header, own version) so that the kernel set, the parameter blocks and the export list of libfa_gfx950.so stay
 * what they are; the error codes are the main header's (FA_OK 0, FA_ERR_INVALID_ARGUMENT -1, FA_ERR_UNSUPPORTED -2, FA_ERR_LAUNCH -3).
 *
 * fa_sink_apply, for every row (b, s, h); fp32 arithmetic, natural log, ONE rounding of out' to the dtype:
 *     lse'  = max(lse, s) + log1p(exp(-|lse - s|))
 *     out'  = out * (1 / (1 + exp(s - lse)))          (exp(+large) = inf gives the factor 0: no NaN)
 *     lse_bwd = lse'                                   (the lse to hand to the backward and to fa_sink_dsink)
 *   - A row whose lse_in is +inf or -inf has NO VISIBLE KEY (+inf is this project's marker, -inf FA3's).  Its out_in row is NOT READ: out' = 0,
 *     lse' = s (the whole softmax mass sits on the sink: the reference's value), lse_bwd = +inf (the backward's P' = exp(S - inf) = 0).
 *   - s = -inf (no sink) is the identity: out' has the bits of out_in, lse' == lse_in -- also on a row without a key, which keeps its marker.
 *   - A factor of exactly 1.0f copies the bits of the row.  A NaN lse or sink is unspecified.
 *   - In place.  out may be exactly out_in, lse exactly lse_in, lse_bwd exactly lse_in (same pointer AND same strides): every element is read and
 *     written by the same lane.  Any other overlap of an output's address range with an input's or another output's is refused (the ranges are compared,
 *     so two interleaved views of one buffer are refused as well).
 *   - The result depends on the values only: bit-identical from run to run and between strided and contiguous tensors.
 *
 * fa_sink_dsink: dsink[h] = - sum over the rows (b, s) whose lse_bwd is finite of exp(sink[h] - lse_bwd) * softmax_d, fp32.
 *   - A row whose lse_bwd is +inf or -inf is skipped and its softmax_d is NOT READ (a backward schedule may leave it unwritten for a row without a key).
 *   - No atomics: a fixed number of workgroups per head (from b * s alone) write partial sums to the caller's workspace, a second launch adds them in
 *     a fixed order.  The result is bit-identical from run to run and between strided and contiguous inputs.
 *   - workspace: at least fa_sink_dsink_workspace_bytes(params) bytes, 4-byte aligned, contents irrelevant before and after.
 *
 * Layout contract (the project's: include/fa_gfx950.h, include/fa_gfx950_combine.h)
 *   - out_in / out: 16-byte aligned; the last (head-dim) stride is 1; every other stride, in bytes, is a multiple of 16 -- checked for dimensions of
 *     more than one element only; a stride of 0 is accepted on an input and refused on an output in a dimension of more than one element;
 *   - lse_in / lse / lse_bwd / softmax_d / dsink: 4-byte aligned, any element strides; sink: aligned to its element, any element stride;
 *   - d % 8 == 0, 8 <= d <= 512; b, s, h >= 0 with b * s * h < 2^31; a call without rows returns FA_OK without a launch and without looking at
 *     pointers or strides (fa_sink_dsink with h > 0 and no rows still writes dsink = 0); every offset is computed in 64 bits.
 *   - A packed (total, h, d) tensor with its (h, total) lse is b = 1, s = total.
 *   A violation returns FA_ERR_INVALID_ARGUMENT with a message naming the argument before anything touches the device.
 *
 * fa_sink_apply launches one kernel, fa_sink_dsink two; neither synchronises with the host, reads device memory on the host or allocates: both
 * can be captured in a HIP graph.
 */
#ifndef FA_GFX950_SINK_H_
#define FA_GFX950_SINK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_SINK_ABI_VERSION 1
/* fa_sink_dsink: workgroups per head at most (the second launch adds that many partials per head in one wave). */
#define FA_SINK_DSINK_MAX_BLOCKS 64

/* 0 and 1 are FA_DTYPE_FP16 / FA_DTYPE_BF16 of the main header; fp32 is a dtype of the sink only. */
enum { FA_SINK_DTYPE_FP16 = 0, FA_SINK_DTYPE_BF16 = 1, FA_SINK_DTYPE_FP32 = 3 };

typedef struct FaSinkApplyParams {
  const void* out_in;           /* (b, s, h, d) under the strides below, dtype `dtype`; rows without a key are not read */
  const float* lse_in;          /* (b, h, s) under its strides                                                           */
  const void* sink;             /* (h), dtype `sink_dtype`                                                               */
  void* out;                    /* (b, s, h, d), dtype `dtype`; may be exactly out_in                                    */
  float* lse;                   /* (b, h, s): lse' (the sink on rows without a key); may be exactly lse_in               */
  float* lse_bwd;               /* (b, h, s): lse', +inf on rows without a key; may be NULL: not written                 */
  int64_t out_in_batch_stride, out_in_row_stride, out_in_head_stride;      /* elements */
  int64_t lse_in_batch_stride, lse_in_row_stride, lse_in_head_stride;      /* elements */
  int64_t out_batch_stride, out_row_stride, out_head_stride;               /* elements */
  int64_t lse_batch_stride, lse_row_stride, lse_head_stride;               /* elements */
  int64_t lse_bwd_batch_stride, lse_bwd_row_stride, lse_bwd_head_stride;   /* elements */
  int64_t sink_stride;                                                     /* elements */
  int32_t dtype;                /* FA_SINK_DTYPE_FP16 / _BF16: out_in and out                                            */
  int32_t sink_dtype;           /* FA_SINK_DTYPE_*                                                                       */
  int32_t b, s, h, d;
} FaSinkApplyParams;

typedef struct FaSinkDsinkParams {
  const float* softmax_d;       /* (b, h, s) under its strides: rowsum(dO * out'), what every backward returns           */
  const float* lse_bwd;         /* (b, h, s) under its strides: fa_sink_apply's lse_bwd                                  */
  const void* sink;             /* (h), dtype `sink_dtype`                                                               */
  float* dsink;                 /* (h), fp32                                                                             */
  void* workspace;              /* workspace_bytes >= fa_sink_dsink_workspace_bytes(params)                              */
  int64_t softmax_d_batch_stride, softmax_d_row_stride, softmax_d_head_stride;   /* elements */
  int64_t lse_bwd_batch_stride, lse_bwd_row_stride, lse_bwd_head_stride;         /* elements */
  int64_t sink_stride, dsink_stride;                                             /* elements */
  int64_t workspace_bytes;
  int32_t sink_dtype;           /* FA_SINK_DTYPE_*                                                                       */
  int32_t b, s, h;
} FaSinkDsinkParams;

int fa_sink_abi_version(void);
int fa_sink_sizeof_apply_params(void);
int fa_sink_sizeof_dsink_params(void);
/* Last error message of the calling thread ("" if none). */
const char* fa_sink_last_error(void);
/* Name of the (first) kernel the calling thread's last call launched ("" if it launched none: a refused call, a call without rows). */
const char* fa_sink_last_kernel_name(void);

/* out' / lse' / lse_bwd from (out, lse, sink): one launch.  `stream` is a hipStream_t. */
int fa_sink_apply(const FaSinkApplyParams* params, void* stream);
/* Bytes of workspace fa_sink_dsink needs for these shapes (b, s, h are read; 0 for a NULL or shapeless block). */
size_t fa_sink_dsink_workspace_bytes(const FaSinkDsinkParams* params);
/* dsink from (softmax_d, lse_bwd, sink): two launches.  `stream` is a hipStream_t. */
int fa_sink_dsink(const FaSinkDsinkParams* params, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA_GFX950_SINK_H_ */
