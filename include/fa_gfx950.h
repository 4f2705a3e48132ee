/*
 * fa_gfx950.h -- C ABI of the MI355X (gfx950 / CDNA4) fused-attention library `libfa_gfx950.so`.
 *
 * This is the drop-in boundary of the hot path: plain pointers, sizes and element strides, no
 * torch / ATen types.  Each entry point replaces one host function of the reference's backend
 * module `flash_attn_2_cuda` (the module `flash_attn/flash_attn_interface.py:13-23` imports):
 *
 *   fa_fwd         <->  mha_fwd         csrc/flash_attn/flash_api.cpp:368-536   (pybind "fwd",        :1537)
 *   fa_varlen_fwd  <->  mha_varlen_fwd  csrc/flash_attn/flash_api.cpp:538-788   (pybind "varlen_fwd", :1538)
 *   fa_bwd         <->  mha_bwd         csrc/flash_attn/flash_api.cpp:800-1008  (pybind "bwd",        :1539)
 *   fa_varlen_bwd  <->  mha_varlen_bwd  csrc/flash_attn/flash_api.cpp:1010-1241 (pybind "varlen_bwd", :1540)
 *   fa_kvcache_append + fa_fwd_kvcache  <->  mha_fwd_kvcache  csrc/flash_attn/flash_api.cpp:1243-1532 (pybind "fwd_kvcache", :1541)
 *
 * The two parameter blocks below are this library's counterpart of the reference's kernel POD
 * `Flash_fwd_params` / `Flash_bwd_params` (csrc/flash_attn/src/flash.h:47-189).  The caller owns
 * every buffer (allocation stays with the framework's caching allocator); the library only
 * enqueues kernels on `stream` and never synchronises.  The torch extension
 * `flash_attn_2_cuda` (flash-attention_amd/csrc/torch_binding.cpp) and the ctypes loader
 * (flash-attention_amd/flash_attn_amd/_cabi.py) are the two in-tree binders; INTEGRATION.md shows
 * the stub a reference maintainer would add.
 *
 * Conventions
 *   - all strides are in ELEMENTS (not bytes); the last (head-dim) stride is 1;
 *   - Layout contract of the fp16 / bf16 entry points (fa_fwd, fa_varlen_fwd, fa_fwd_kvcache, fa_bwd, fa_varlen_bwd, the 16-bit fa_kvcache_append,
 *     fa_rotary; the fp8 entry points and the (576, 512) pair state theirs below): the kernels move every row in 16-byte chunks, so
 *       * every tensor pointer (q, k, v, o, dout, dq, dk, dv, knew, vnew, kcache, vcache, x, y) is 16-byte aligned;
 *       * every batch, row and head stride is a multiple of 8 elements WHEN ITS DIMENSION HAS MORE THAN ONE ELEMENT.  The stride of a dimension of one
 *         element (one KV head, B = 1, one query row) is never multiplied by a non-zero index: any value is accepted and none is relied upon.  Extents
 *         that are not parameters (cache entries behind cache_batch_idx, pages, the key rows of a packed batch) count as more than one;
 *       * a stride of 0 is accepted for inputs (a tensor expanded over the batch or the heads);
 *       * outputs (o, dq, dk, dv, kcache, vcache of the append, y) have non-zero strides in every dimension of more than one element (the launching
 *         calls check this; the queries, which write nothing, do not).
 *     Within that, the tensors of one call are independent: each has its own base and its own (batch, row, head) strides (column slices of one fused
 *     projection, transposed (B,H,S,D) / (S,B,H,D) buffers, views of a packed gradient, padded heads, every second row ...).  A violation returns
 *     FA_ERR_INVALID_ARGUMENT with a message naming the entry point and the tensor, before anything touches the device; fa_fwd_schedule_query,
 *     fa_bwd_dq_schedule_query and fa_bwd_plan_query return the same error, fa_fwd_workspace_bytes / fa_bwd_workspace_bytes return 0;
 *   - q (B,Sq,H,D), k/v (B,Sk,Hk,D), o like q; varlen: q (total_q,H,D), k/v (total_k,Hk,D) and
 *     batch strides are ignored; sequence b owns rows cu_seqlens[b] .. cu_seqlens[b+1]-1
 *     (reference csrc/flash_attn/src/block_info.h:12-45);
 *   - softmax_lse is fp32 (B,H,Sq) or, varlen, (H,total_q); natural log of sum_j exp(scale*s_ij);
 *     rows without any visible key give out = 0, lse = +inf (reference softmax.h:179-180);
 *   - window_left / window_right < 0 mean unbounded; is_causal forces window_right = 0; masks are
 *     aligned to the bottom-right corner (reference flash_attn_interface.py:1175-1189);
 *   - head dim d: any multiple of 8 up to 256, forward and backward.  Kernels are built for 32 / 64 / 96 / 128 / 192 / 256 (the reference's
 *     set, static_switch.h:92-110); a size in between runs the next built size's kernels with a run-time column bound: the 16-byte chunks
 *     behind d are read as zeros and never stored, so q / k / v / out / gradients keep their own row pitch -- no padded copies (the reference
 *     rounds internally the same way, flash_api.cpp:458,872);
 *   - v may have a head dim of its own (FaFwdParams::d_v): q / k (.., 192), v / o (.., 128) is built (fa_fwd / fa_varlen_fwd: plain attention under
 *     causal / window masks, MHA / GQA / MQA, seqused_q / seqused_k; softmax_scale is the caller's -- the binders default to d ** -0.5, d = q's head dim).  Any
 *     other pair with d_v != d, and this pair with dropout, softcap, ALiBi, return_softmax, block_table, leftpad_k, a KV cache or FP8, returns
 *     FA_ERR_UNSUPPORTED with a message naming both head dims or the argument;
 *   - absorbed MLA decode (fa_fwd_kvcache only): d = 576 with d_v = 512 -- q (B,Sq,H,576), a latent cache k (.., Hk, 576) = 512 latent + 64 rotary channels,
 *     o (B,Sq,H,512) -- where v IS the first 512 channels of the k rows: the caller passes the view k_cache[..., :512], i.e. v == k with equal batch / row /
 *     head strides, and every cache row is read from HBM once for both products.  Anything else as v returns FA_ERR_UNSUPPORTED ("V must be the first 512
 *     channels of K").  bf16 / fp16, any H % Hk == 0 (the query heads of a KV group are always packed into the rows of 64-row blocks), any seqlen_q, k row
 *     stride >= 576, all q / k / o strides multiples of 8 elements, q / k 16-byte aligned; seqused_k (+ seqused_k_add), cache_batch_idx, block_table (pages
 *     of a multiple of 256 keys), causal / window masks aligned to each entry's own length, num_splits with fp32 partials of width 512
 *     (fa_fwd_workspace_bytes: (512 + 1) * 4 bytes per row and split; keys are split while H / Hk * seqlen_q <= 128).  FA_ERR_UNSUPPORTED naming (576, 512)
 *     or the argument for leftpad_k, ALiBi, softcap, the fp8 entry points, fa_fwd / fa_varlen_fwd and the backward; d = 576 with d_v = 0 or 576 stays
 *     "at most 256".  At most 64 key splits (as on every KV-cache path: the merge reads one split per lane).  fa_kvcache_append writes such rows once (below);
 *   - return value 0 = enqueued; negative = FA_ERR_* (message via fa_last_error()).
 */
#ifndef FA_GFX950_H_
#define FA_GFX950_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_ABI_VERSION 6

enum { FA_DTYPE_FP16 = 0, FA_DTYPE_BF16 = 1, FA_DTYPE_FP8_E4M3 = 2 /* OCP e4m3 (float8_e4m3fn): fa_fwd_fp8 / fa_varlen_fwd_fp8 / fa_fwd_kvcache_fp8 and fa_kvcache_append only */ };

enum {
  FA_OK = 0,
  FA_ERR_INVALID_ARGUMENT = -1, /* shape/dtype/stride contract violated                     */
  FA_ERR_UNSUPPORTED = -2,      /* valid in the reference but not built here (see message)   */
  FA_ERR_LAUNCH = -3,           /* hipLaunchKernel failed                                     */
  FA_ERR_WORKSPACE = -4         /* workspace missing or too small                             */
};

typedef struct FaFwdParams {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* softmax_lse;           /* (B,H,Sq) or varlen (H,total_q) */
  int64_t q_batch_stride, q_row_stride, q_head_stride;
  int64_t k_batch_stride, k_row_stride, k_head_stride;
  int64_t v_batch_stride, v_row_stride, v_head_stride;
  int64_t o_batch_stride, o_row_stride, o_head_stride;
  const int32_t* cu_seqlens_q;  /* NULL => fixed-length batch          */
  const int32_t* cu_seqlens_k;  /* NULL => fixed-length batch          */
  const int32_t* seqused_k;     /* optional (B): keys actually used     */
  const float* alibi_slopes;    /* optional (H) or (B,H) fp32           */
  int64_t alibi_batch_stride;   /* 0 when slopes are (H)                */
  int32_t b, h, h_k, d;
  int32_t seqlen_q, seqlen_k;   /* fixed: exact; varlen: max_seqlen_*   */
  int32_t total_q;              /* varlen: rows of q; fixed: b*seqlen_q */
  int32_t dtype;                /* FA_DTYPE_*                           */
  int32_t is_causal;
  int32_t window_left, window_right;
  float softmax_scale;
  float softcap;                /* 0 = off                              */
  int32_t seqused_k_add;        /* added to seqused_k[b] (keys appended in the same call)            */
  /* KV-cache extensions (NULL / 0 otherwise) */
  const int32_t* cache_batch_idx;   /* fa_fwd_kvcache, optional (B): batch entry -> row of the cache */
  const int32_t* block_table;       /* fa_fwd_kvcache / fa_varlen_fwd, optional (B, max_blocks) int32: paged K/V, k/v are
                                       (num_blocks, page, Hk, D) and k/v_batch_stride is the page stride */
  int64_t block_table_batch_stride;
  int32_t page_block_size;          /* keys per page, multiple of 256 (reference flash_api.cpp:1318)  */
  int32_t num_splits;               /* fa_fwd_kvcache: 0 = heuristic, 1 = no split, >1 = split the keys this many ways */
  float p_dropout;                  /* probability to DROP, in [0, 1); 0 = off                         */
  int32_t d_v;                      /* head dim of v / o when it differs from d (took the place of a reserved field; 0 = d).  fa_fwd_kvcache: only d = 576,
                                       d_v = 512 with v == k (see above).  fa_fwd / fa_varlen_fwd:
                                       only the pair d = 192, d_v = 128 (DeepSeek-V2/V3 multi-head latent attention: 128 "nope" + 64 rotary q/k
                                       channels, 128 v channels; the reference's hopper/flash_api.cpp:782-786): v is (.., Hk, d_v), o (.., H, d_v) */
  /* dropout (p_dropout > 0): */
  const uint64_t* rng_state;        /* device, 2 x u64 {seed, offset} (reference rng_state, flash_api.cpp:496-515) */
  uint8_t* randval;                 /* optional out: the random byte of every (query, key) pair; a pair is KEPT iff
                                       byte <= floor(255*(1-p_dropout)) (the ROCm backend's return_softmax payload,
                                       csrc/flash_attn_ck/mha_fwd.cpp:275-279); (B,H,Sq,Sk) or varlen (H,total_q,max_seqlen_k) */
  int64_t randval_batch_stride, randval_head_stride, randval_row_stride;
  /* split-KV scratch (fa_fwd_kvcache): fa_fwd_workspace_bytes() bytes, 256-B aligned; may be NULL if that is 0 */
  void* workspace;
  int64_t workspace_bytes;
  const int32_t* leftpad_k;         /* fa_varlen_fwd / fa_fwd_kvcache, optional (B): the keys of entry b start at row leftpad_k[b];
                                       lengths (seqused_k / cu_seqlens_k) count from row 0 (reference block_info.h:17-36);
                                       not together with block_table */
  const int32_t* seqused_q;         /* ABI v6, fa_fwd / fa_varlen_fwd, optional (B): only the first seqused_q[b] query rows of entry b exist
                                       (the rest of its rows -- cu_seqlens_q[b+1] - cu_seqlens_q[b], or seqlen_q -- are padding: never
                                       read, their o / softmax_lse rows never written).  With cu_seqlens_q[b] = b*S + first valid row and
                                       seqused_q / seqused_k = the valid lengths, a PADDED (B,S,H,D) batch runs in place: the gather /
                                       scatter passes of the reference's unpad_input / pad_input (flash_attn/bert_padding.py:98-128,
                                       204-218) disappear */
} FaFwdParams;

/* Append step of the KV-cache path: copy knew/vnew (B, S_new, Hk, D) into the cache at rows
 * seqlens_k[b] .. seqlens_k[b]+S_new-1 of cache row cache_batch_idx[b] (or page-table addressed).
 * For ANY dtype and d: when vnew == knew and vcache == kcache with equal batch / row / head strides on both sides (the values are a view of the key
 * rows, e.g. the absorbed MLA cache), the key copy has written every byte and the V copy is skipped -- such a call used to write the same bytes twice. */
typedef struct FaKvAppendParams {
  const void* knew;
  const void* vnew;
  void* kcache;
  void* vcache;
  int64_t knew_batch_stride, knew_row_stride, knew_head_stride;
  int64_t vnew_batch_stride, vnew_row_stride, vnew_head_stride;
  int64_t kcache_batch_stride, kcache_row_stride, kcache_head_stride;
  int64_t vcache_batch_stride, vcache_row_stride, vcache_head_stride;
  const int32_t* seqlens_k;         /* (B) current lengths; NULL => append at row 0                  */
  const int32_t* cache_batch_idx;   /* optional                                                       */
  const int32_t* block_table;       /* optional (paged cache)                                         */
  int64_t block_table_batch_stride;
  int32_t page_block_size;
  int32_t b, seqlen_new, h_k, d;
  int32_t dtype;
  int32_t reserved[2];
} FaKvAppendParams;

/* Rotary position embedding of x (B, S, H, D) into y (same shape, may alias x): the first rotary_dim channels of
 * every row are rotated by the angle row of position seqlen_offsets[b] + (per_token ? s : 0)
 * (reference flash_fwd_kernel.h:640-720 Append_KV rotary, csrc/flash_attn/src/rotary.h; Python
 * flash_attn/layers/rotary.py apply_rotary_emb).  cos/sin: (seqlen_ro, rotary_dim/2), same dtype as x. */
typedef struct FaRotaryParams {
  const void* x;
  void* y;
  const void* cos;
  const void* sin;
  const int32_t* seqlen_offsets;   /* (B) or NULL (= 0) */
  int64_t x_batch_stride, x_row_stride, x_head_stride;
  int64_t y_batch_stride, y_row_stride, y_head_stride;
  int64_t cos_row_stride;          /* elements between consecutive positions of cos / sin */
  int32_t b, s, h, d;
  int32_t rotary_dim;              /* multiple of 16, <= d */
  int32_t seqlen_ro;               /* rows of cos / sin */
  int32_t interleaved;             /* 1: pairs (2t, 2t+1) (GPT-J); 0: pairs (t, t + rotary_dim/2) (GPT-NeoX) */
  int32_t per_token;               /* 1: row s sits at position offset + s; 0: every row at position offset */
  int32_t dtype;
  int32_t reserved[3];
} FaRotaryParams;

typedef struct FaBwdParams {
  const void* dout;
  const void* q;
  const void* k;
  const void* v;
  const void* o;
  const float* softmax_lse;     /* as written by fa_fwd                */
  void* dq;
  void* dk;
  void* dv;
  float* softmax_d;             /* out: rowsum(dO*O), fp32, same shape/indexing as softmax_lse */
  void* workspace;              /* fa_bwd_workspace_bytes() bytes, 256-B aligned, may be NULL if that is 0 */
  int64_t workspace_bytes;
  int64_t do_batch_stride, do_row_stride, do_head_stride;
  int64_t q_batch_stride, q_row_stride, q_head_stride;
  int64_t k_batch_stride, k_row_stride, k_head_stride;
  int64_t v_batch_stride, v_row_stride, v_head_stride;
  int64_t o_batch_stride, o_row_stride, o_head_stride;
  int64_t dq_batch_stride, dq_row_stride, dq_head_stride;
  int64_t dk_batch_stride, dk_row_stride, dk_head_stride;
  int64_t dv_batch_stride, dv_row_stride, dv_head_stride;
  const int32_t* cu_seqlens_q;
  const int32_t* cu_seqlens_k;
  const float* alibi_slopes;
  int64_t alibi_batch_stride;
  int32_t b, h, h_k, d;
  int32_t seqlen_q, seqlen_k;
  int32_t total_q, total_k;
  int32_t dtype;
  int32_t is_causal;
  int32_t window_left, window_right;
  float softmax_scale;
  float softcap;
  int32_t deterministic;        /* accepted; this implementation is always deterministic */
  float p_dropout;              /* as in the forward call                                  */
  int32_t d_v;                  /* head dim of v / o / dout / dv when it differs from d (took the first reserved field; 0 = d), as FaFwdParams::d_v */
  int32_t reserved[2];
  const uint64_t* rng_state;    /* device {seed, offset} the forward used (p_dropout > 0) */
  const int32_t* seqused_q;     /* ABI v6, optional (B): as FaFwdParams::seqused_q; dq rows past it are not written */
  const int32_t* seqused_k;     /* ABI v6, optional (B): keys of entry b in use.  In the backward it can only SHORTEN an entry: the length is
                                   min(seqused_k[b], the cu_seqlens_k length) (fixed-length: min(seqused_k[b], seqlen_k)) -- the key-block work
                                   list is sized from cu_seqlens_k, so a longer value could not be honoured by every kernel (round 5).  Round 6: the
                                   forward applies the same rule inside a packed batch (cu_seqlens_k without a block table): min(seqused_k[b] +
                                   seqused_k_add, the cu_seqlens_k length); only against a KV cache (no cu_seqlens_k, or a paged one) does
                                   seqused_k REPLACE the length.  A forward / backward pair therefore always sees the same keys; dk / dv rows
                                   past it are not written */
} FaBwdParams;

/* Descale factors of the FP8 forwards (fa_fwd_fp8 / fa_varlen_fwd_fp8 / fa_fwd_kvcache_fp8): fp32 device tensors of shape (B, Hk) -- per KV head, FA3's
 * q_descale / k_descale / v_descale (hopper/flash_api.cpp) -- with any strides (in elements).  A NULL pointer means 1.0. */
typedef struct FaFp8Params {
  const float* q_descale;
  const float* k_descale;
  const float* v_descale;
  int64_t q_descale_batch_stride, q_descale_head_stride;
  int64_t k_descale_batch_stride, k_descale_head_stride;
  int64_t v_descale_batch_stride, v_descale_head_stride;
} FaFp8Params;

/* ABI version of the loaded library (== FA_ABI_VERSION of the header it was built from). */
int fa_abi_version(void);
/* sizeof() of the two parameter blocks as the library sees them (binder self-check). */
int fa_sizeof_fwd_params(void);
int fa_sizeof_bwd_params(void);
int fa_sizeof_kvappend_params(void);
int fa_sizeof_rotary_params(void);
int fa_sizeof_fp8_params(void);
/* Last error message of the calling thread ("" if none). */
const char* fa_last_error(void);

/* Run-time knobs (FA_FWD_NW, FA_RESCALE_THR, FA_VARLEN_LIST, FA_IL_SCHED, FA_BWD_DQ_NW; INTEGRATION.md "Run-time knobs")
 * are read from the environment once per process; this re-reads them (tests / A-B tools after changing the environment). */
void fa_knobs_reload(void);
/* Which kernels the calling thread's last fa_fwd* / fa_bwd* call enqueued (for tests and the benchmark's labels; the
 * reference exposes nothing comparable -- its dispatch is compile-time, flash_fwd_launch_template.h).  Fills up to n of
 * FA_SCHEDULE_FIELDS int32: {forward kernel id (0 none, 1 lock-step fa_fwd_kernel, 2 pipelined fa_fwd_il_kernel,
 * 3 64-rows-per-wave fa_fwd_w64_kernel, 4 FP8 fa_fwd_fp8_kernel, 5 FP8 KV-cache fa_fwd_fp8_kv_kernel, 6 fa_fwd_dv_kernel: v / o head dim of its own, 7 fa_fwd_mla_kernel: absorbed MLA decode 576 / 512), waves per workgroup (16 = 8-wave ping-pong), feature variant, key splits,
 * varlen work list used, head dim, bf16, dQ-kernel waves, backward work lists used, backward spilled dS (5 contractions),
 * query heads packed into the rows of a block (fa_fwd_kvcache, 1 = none), dK/dV schedule (8 waves x 32 keys, 4 at head dim 256,
 * or 64 = 4 waves x 64 keys), head dim of v / o (= head dim unless FaFwdParams::d_v set it)}; returns FA_SCHEDULE_FIELDS (fields are only ever appended). */
#define FA_SCHEDULE_FIELDS 13
int fa_last_schedule(int32_t* out, int n);
/* Name of the forward kernel instantiation of that call, e.g. "fa::fa_fwd_il_kernel<bf16,128,4,3>" ("" if none). */
const char* fa_last_kernel_name(void);
/* Launch log (tests; FA_DEBUG_LAUNCH_LOG=1 in the environment when the knobs are read, else nothing is recorded): the __global__ instantiations the calling
 * thread's last launching call (fa_fwd*, fa_varlen_fwd*, fa_fwd_kvcache*, fa_bwd, fa_varlen_bwd, fa_rotary, fa_kvcache_append, fa_set_rng_state) enqueued, in launch
 * order, as the (mangled) symbol names of the code objects, each followed by '\n'.  Writes what fits into buf[0..n) (whole lines, 0-terminated) and returns the
 * bytes the whole text needs, terminator included (1 = empty log): call again with a larger buffer if that exceeds n. */
int fa_launch_log(char* buf, int n);
/* Host logic only (no launch, no pointer is dereferenced -- pointers count as flags: alibi_slopes, block_table, cu_seqlens_q, seqused_q): the forward
 * schedule fa_fwd (varlen = 0) / fa_varlen_fwd (varlen = 1) would run for these parameters, as an FA_FWD_NW code -- 64 = 64-rows-per-wave kernel,
 * 34 / 38 = software-pipelined kernel with 4 / 8 waves, 4 / 8 / 16 = lock-step kernel -- after the feature / head-dim / head-packing fallbacks; and the dQ
 * schedule of the backward (4 / 8 waves x 32 rows, 64 = 4 waves x 64 rows).  Negative = FA_ERR_*.  For tests of the dispatch on a box without a GPU. */
int fa_fwd_schedule_query(const FaFwdParams* params, int varlen);
int fa_bwd_dq_schedule_query(const FaBwdParams* params);
/* Which backward a fixed-length call runs and how its workspace is laid out (round 6; host logic only, for tests of the dispatch on a box without a GPU):
 * out[0] = 0 the recomputing pair (7 contractions, no dS workspace), 3 = the fused launch (dK/dV + dQ = dS.K, FA_BWD_MODE=3 or the default table; out[1] = launches
 * = chunks of whole batch entries, out[2] = batch entries per chunk, out[7] = MiB of workspace),
 * 5 = the chunked 5-contraction backward (FA_BWD_MODE=5); for 5: out[1] = chunks, out[2] = XCD rounds (8 units) per chunk, out[3] = dS sub-tiles (2 KB) per
 * head with packed rows, out[4] = 64-key pairs per row, out[5] / out[6] = the row packing's a / jb (csrc/fa_device.h ds_row_start), out[7] = MiB per slot.
 * For 0 (the pair): out[3] = virtual kv heads per GQA group when the dK/dV kernels split the groups to fill the chip (0 = unsplit), out[7] = MiB of workspace for the partials.
 * Returns the number of fields (8) or a negative FA_ERR_*. */
int fa_bwd_plan_query(const FaBwdParams* params, int32_t* out, int n);

/* Forward, fixed-length batch.  cu_seqlens_* must be NULL.  `stream` is a hipStream_t. */
int fa_fwd(const FaFwdParams* params, void* stream);
/* Forward, packed variable-length batch.  cu_seqlens_q/k must be non-NULL device int32 (b+1). */
int fa_varlen_fwd(const FaFwdParams* params, void* stream);
/* Forward on FP8 inputs (FA3's fp8 forward): q / k / v are OCP e4m3 (dtype FA_DTYPE_FP8_E4M3; strides multiples of 16 bytes, pointers 16-byte
 * aligned), o is bf16 (strides multiples of 8 elements).  S = softmax_scale * q_descale * k_descale * q.k^T on the exact fp8 values, P = softmax(S)
 * rounded to e4m3, o = P.(v_descale * v); softmax_lse as fa_fwd.  fp8 may be NULL (all descales 1).  Causal / window masks, MHA / GQA / MQA,
 * head dims 64 and 128.  FA_ERR_UNSUPPORTED (with a message naming it) for any other head dim, softcap, ALiBi, dropout, return_softmax,
 * seqused_q / seqused_k, leftpad_k, block_table and the KV-cache arguments (those belong to fa_fwd_kvcache_fp8); there is no fp8 backward.
 * fa_varlen_fwd_fp8: packed batch as fa_varlen_fwd (the workspace of fa_fwd_workspace_bytes holds the work list of an uneven batch). */
int fa_fwd_fp8(const FaFwdParams* params, const FaFp8Params* fp8, void* stream);
int fa_varlen_fwd_fp8(const FaFwdParams* params, const FaFp8Params* fp8, void* stream);
/* Inference forward of e4m3 queries against an e4m3 KV cache (FA3's flash_attn_with_kvcache with q_descale / k_descale / v_descale): the contract of
 * fa_fwd_fp8 -- layout rules, math, bf16 o, fp32 softmax_lse, descales (B, Hk) indexed by the batch entry of q, not by the cache row -- with the cache
 * arguments of fa_fwd_kvcache: seqused_k (+ seqused_k_add), cache_batch_idx, block_table (pages of a multiple of 256 keys; seqlen_k = max_blocks * page),
 * num_splits and the workspace of fa_fwd_workspace_bytes; masks are aligned to each entry's own length; the query heads of a KV group are packed into
 * the rows of a block when group * seqlen_q <= 128.  Head dims 64 and 128.  FA_ERR_UNSUPPORTED (with a message naming it) for softcap, ALiBi,
 * leftpad_k, dropout / return_softmax, seqused_q and any other head dim.  New keys are appended first with fa_kvcache_append (dtype FA_DTYPE_FP8_E4M3:
 * a byte copy, d a multiple of 16, strides multiples of 16 bytes, pointers 16-byte aligned) -- the caller quantises them with the cache's scale;
 * fa_rotary refuses e4m3 (rotating quantised values needs a requantisation nobody has defined). */
int fa_fwd_kvcache_fp8(const FaFwdParams* params, const FaFp8Params* fp8, void* stream);
/* Inference forward against a KV cache: fa_fwd plus seqused_k (cache_seqlens), cache_batch_idx and/or a
 * paged cache (block_table).  k/v point at the cache.  No backward.  d = 576, d_v = 512, v == k: the absorbed MLA decode (Conventions above). */
int fa_fwd_kvcache(const FaFwdParams* params, void* stream);
/* Writes the new keys/values into the cache (call before fa_fwd_kvcache with seqused_k_add = seqlen_new). */
int fa_kvcache_append(const FaKvAppendParams* params, void* stream);
/* Writes {seed, offset} to a device rng_state (2 x u64) in stream order (binder helper for p_dropout > 0). */
int fa_set_rng_state(uint64_t seed, uint64_t offset, uint64_t* rng_state, void* stream);
/* Bytes of split-KV scratch fa_fwd_kvcache / fa_fwd_kvcache_fp8 need for this problem with params->num_splits (0 is possible). */
int64_t fa_fwd_workspace_bytes(const FaFwdParams* params);
/* Rotary embedding of q / new keys ahead of fa_kvcache_append + fa_fwd_kvcache (y may alias x). */
int fa_rotary(const FaRotaryParams* params, void* stream);
/* Bytes of scratch the backward can use for this problem (0 is possible).  For fa_bwd (fixed-length batches) the scratch is the dS area of the 5-contraction
 * launches (up to 1.25 GiB by default; FA_BWD_MODE / FA_BWD_DS_CAP_MB / FA_BWD_C5_CAP_MB): a speed-up, not a requirement -- called with workspace = NULL or fewer
 * bytes, fa_bwd runs the recomputing pair, which needs none (both binders do exactly that when their allocator is out of memory).  For fa_varlen_bwd it holds the
 * work lists of an uneven batch (a few KB). */
int64_t fa_bwd_workspace_bytes(const FaBwdParams* params);
/* Backward, fixed-length batch: writes dq, dk, dv (caller-allocated) and softmax_d. */
int fa_bwd(const FaBwdParams* params, void* stream);
/* Backward, packed variable-length batch. */
int fa_varlen_bwd(const FaBwdParams* params, void* stream);
/* Opt-in fused backward (FA_BWD_MODE=3) only: after fa_bwd with the SAME params, waits for `stream` and reads the launch's error flag from the workspace.
   0 = the launch completed its hand-offs (or the call did not take the fused path), FA_ERR_LAUNCH = a dQ hand-off timed out: that 256-row block of dq was
   not written, the gradients of this call must be discarded.  Both binders call it after every fused backward (the mode is experimental; the default
   backward has no cross-workgroup hand-off and nothing to check). */
int fa_bwd_fused_status(const FaBwdParams* params, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA_GFX950_H_ */
