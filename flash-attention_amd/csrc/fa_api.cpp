// C-ABI entry points of libfa_gfx950.so (declared in include/fa_gfx950.h).
//
// Host layer of the hot path: validates the contract, normalises (causal, window) exactly as the
// reference host functions do, fills the device-side parameter block and enqueues the kernels.
// Behavioural spec: reference csrc/flash_attn/flash_api.cpp -- mha_fwd :368-536,
// mha_varlen_fwd :538-788, mha_bwd :800-1008, mha_varlen_bwd :1010-1241, set_params_fprop :44-177
// (window/causal normalisation :155-162 and :422-427).  No ATen here: buffers are caller-owned.
// What a call runs -- the schedule heuristics and their measurements (fwd_schedule_nw, pack_group, choose_splits, bwd_dq_schedule, bwd_fused_by_table,
// bwd_c5_plan, bwd_gsplit_plan, ...) -- is decided once per call in fa_plan.h (plan_fwd / plan_bwd); the functions here validate, fill and launch.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../include/fa_gfx950.h"
#include "fa_device.h"
#include "fa_kernel_params.h"
#include "fa_launch.h"
#include "fa_plan.h"

namespace {

thread_local char g_err[512] = {0};

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int env_int(const char* name, int dflt) {
  const char* s = getenv(name);
  return (s && *s) ? atoi(s) : dflt;
}

// Environment knobs are read once per process (getenv on every launch races with setenv and costs a libc lock);
// fa_knobs_reload() re-reads them.  Old snapshots are never freed (a handful of bytes per reload).
std::atomic<const fa::Knobs*> g_knobs{nullptr};
const fa::Knobs* read_knobs() {
  fa::Knobs* k = new fa::Knobs();
  k->fwd_nw = env_int("FA_FWD_NW", 0);
  const char* t = getenv("FA_RESCALE_THR");
  k->rescale_thr = (t && *t) ? (float)atof(t) : 8.f;
  if (!(k->rescale_thr >= 0.f) || k->rescale_thr > 16.f) k->rescale_thr = 0.f;
  k->varlen_list = env_int("FA_VARLEN_LIST", 1);
  k->il_sched = env_int("FA_IL_SCHED", 3);
  k->bwd_dq_nw = env_int("FA_BWD_DQ_NW", 0);
  k->bwd_mode = env_int("FA_BWD_MODE", 0);
  k->bwd_dkdv = env_int("FA_BWD_DKDV", 0);
  k->bwd_ds_cap_mb = env_int("FA_BWD_DS_CAP_MB", 8192);
  k->bwd_fused_check = env_int("FA_BWD_FUSED_CHECK", 0);
  k->bwd_c5_cap_mb = std::max(16, std::min(65536, env_int("FA_BWD_C5_CAP_MB", 1024)));
  k->fz_line = std::max(1, std::min(64, env_int("FA_FZ_LINE", 32)));
  k->bwd_gsplit = env_int("FA_BWD_GSPLIT", 1);
  k->w64_persist = env_int("FA_W64_PERSIST", 1);
  k->strict = env_int("FA_STRICT", 0);
  k->dkdv_prescale = env_int("FA_DKDV_PRESCALE", 0);
  k->bwd_fuse_delta = env_int("FA_BWD_FUSE_DELTA", 1);
  k->pack_gqa = env_int("FA_PACK_GQA", 1);
  k->fp8_kv_ring = env_int("FA_FP8_KV_RING", 4);
  if (k->fp8_kv_ring < 2 || k->fp8_kv_ring > 4) k->fp8_kv_ring = 4;
  k->launch_log = env_int("FA_DEBUG_LAUNCH_LOG", 0);
  if (k->strict) k->rescale_thr = 0.f;
  return k;
}

}  // namespace
namespace fa {
const Knobs& knobs() {
  const Knobs* k = g_knobs.load(std::memory_order_acquire);
  if (!k) {
    const Knobs* fresh = read_knobs();
    if (g_knobs.compare_exchange_strong(k, fresh, std::memory_order_acq_rel)) k = fresh;
    else delete fresh;
  }
  return *k;
}
LastSchedule& last_schedule() {
  thread_local LastSchedule ls{};
  return ls;
}
// Launch log (fa_launch.h): host pointers of the kernels this thread's last C ABI call enqueued.  A call launches a handful of kernels (the 5-contraction backward
// one per chunk); past the capacity only the count goes on and fa_launch_log says so.
namespace {
constexpr int kLaunchLogCap = 256;
struct LaunchLog { int n; const void* kern[kLaunchLogCap]; };
LaunchLog& launch_log() {
  thread_local LaunchLog l{};
  return l;
}
}  // namespace
void launch_log_push(const void* kern) {
  LaunchLog& l = launch_log();
  if (l.n < kLaunchLogCap) l.kern[l.n] = kern;
  ++l.n;
}
void launch_log_clear() { launch_log().n = 0; }
int launch_log_count() { return launch_log().n; }
const void* launch_log_at(int i) { return (i >= 0 && i < launch_log().n && i < kLaunchLogCap) ? launch_log().kern[i] : nullptr; }
}  // namespace fa
namespace {

// dropout fields shared by the forward and backward parameter blocks
int check_dropout(float p_dropout, const void* rng_state) {
  if (!(p_dropout >= 0.f) || p_dropout >= 1.f) return fail(FA_ERR_INVALID_ARGUMENT, "p_dropout must be in [0, 1)");
  if (p_dropout > 0.f && !rng_state) return fail(FA_ERR_INVALID_ARGUMENT, "p_dropout > 0 needs a device rng_state {seed, offset}");
  return FA_OK;
}
template <typename K> void fill_dropout(K& k, float p_dropout, const uint64_t* rng_state) {
  if (p_dropout > 0.f) {
    k.rng = rng_state;
    const float p_keep = 1.0f - p_dropout;  // single precision throughout, as csrc/flash_attn_ck/mha_fwd.cpp derives its uint8 threshold
    k.drop_thr8 = (uint32_t)std::floor(p_keep * 255.0f);
    k.rp_keep = 1.f / (1.f - p_dropout);
  }
}

// Launches the schedule pre-pass of a packed forward into the caller's workspace and points k at the list; without a list in the plan (a dense enough
// batch, or no workspace) k is left alone.
int fwd_work_list(const FaFwdParams* a, const FwdPlan& pl, void* stream, fa::FwdK& k) {
  if (!pl.list) return FA_OK;
  fa::SchedK sk{};
  sk.cu_a = a->cu_seqlens_q; sk.cu_o = a->cu_seqlens_k; sk.seqused_o = a->seqused_k;
  sk.list = (int2*)a->workspace; sk.nb = a->b; sk.blk = pl.bm; sk.bound = (int)pl.list_entries; sk.wl = pl.wl; sk.wr = pl.wr; sk.keys_blocked = 0;
  sk.work_shift = fa::sched_work_shift(a->seqlen_k);
  if (fa::launch_varlen_schedule(sk, (hipStream_t)stream) != 0)
    return fail(FA_ERR_LAUNCH, "schedule kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
  k.work_list = (const int2*)a->workspace;
  k.work_bound = (int)pl.list_entries;
  return FA_OK;
}

int check_common(int b, int h, int h_k, int d, int dtype, float softcap, int d_v = 0) {
  if (b <= 0) return fail(FA_ERR_INVALID_ARGUMENT, "batch size must be positive");
  if (h <= 0 || h_k <= 0 || h % h_k != 0)
    return fail(FA_ERR_INVALID_ARGUMENT, "Number of heads in key/value must divide number of heads in query");
  if (d <= 0 || (d > 256 && !mla_pair(d, d_v)) || d % 8 != 0)   // (576 only together with d_v = 512: check_value_dim says where that pair runs)
    return fail(FA_ERR_INVALID_ARGUMENT, "head dimension must be a multiple of 8 and at most 256");
  if (dtype != FA_DTYPE_FP16 && dtype != FA_DTYPE_BF16)
    return fail(FA_ERR_INVALID_ARGUMENT, "FlashAttention only supports fp16 and bf16 data type");
  if (softcap < 0.f) return fail(FA_ERR_INVALID_ARGUMENT, "softcap must be non-negative");
  return FA_OK;
}

// Layout contract of the 16-bit entry points (fa_gfx950.h, "Layout contract"): every kernel moves a row in 16-byte chunks -- ld_global_16B, the
// buffer_load_dwordx4 .. lds of the 64-per-wave kernels, 16-byte stores -- from base + (b * bs + row * rs + head * hs) * 2, so every pointer is 16-byte
// aligned and every stride that is multiplied by a non-zero index a multiple of 8 elements.  n_batch / n_rows / n_heads are the extents the strides walk
// (kMany where the extent is not a parameter: cache entries behind a batch index, pages, the rows of a packed batch); a dimension of one element is
// never stepped, so its stride is neither checked nor used.  A stride of 0 (an expanded input) is a multiple of 8; an output written through it would
// have several (b, row, head) share one address.  NULL tensors are skipped: the entry points refuse them by name, the sizing queries do not need them.
constexpr int64_t kMany = 2;
struct TensorLayout {
  const char* name; const void* p;
  int64_t bs, rs, hs;
  int64_t n_batch, n_rows, n_heads;
  bool output;
};
int check_layouts(const char* fn, std::initializer_list<TensorLayout> ts) {
  for (const TensorLayout& t : ts) {
    if (!t.p) continue;
    if (((uintptr_t)t.p & 15u) != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s must be 16-byte aligned (the kernels move 16-byte chunks)", fn, t.name);
    const struct { const char* what; int64_t stride, n; } dims[] = {{"batch", t.bs, t.n_batch}, {"row", t.rs, t.n_rows}, {"head", t.hs, t.n_heads}};
    for (const auto& d : dims) {
      if (d.n <= 1) continue;
      if (d.stride % 8 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: the %s stride of %s (%lld elements) must be a multiple of 8 elements = 16 bytes", fn, d.what, t.name, (long long)d.stride);
      if (t.output && d.stride == 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: the %s stride of the output %s must be non-zero", fn, d.what, t.name);
    }
  }
  return FA_OK;
}
// fa_fwd / fa_varlen_fwd / fa_fwd_kvcache and the queries that mirror them (dtype fp16 / bf16; the MLA pair and the fp8 entry points have checks of their own)
// (writes = false: a query, which enqueues nothing -- the rule on output strides belongs to the launching calls)
int check_fwd_layout(const char* fn, const FaFwdParams* a, bool varlen, bool kvcache, bool writes = true) {
  const bool packed_k = varlen && !a->block_table;
  const int64_t nb = varlen ? 1 : a->b, rows_q = varlen ? a->total_q : a->seqlen_q;
  const int64_t nb_k = packed_k ? 1 : (kvcache || a->block_table) ? kMany : a->b;
  const int64_t rows_k = packed_k ? kMany : a->block_table ? a->page_block_size : a->seqlen_k;
  return check_layouts(fn, {{"q", a->q, a->q_batch_stride, a->q_row_stride, a->q_head_stride, nb, rows_q, a->h, false},
                            {"k", a->k, a->k_batch_stride, a->k_row_stride, a->k_head_stride, nb_k, rows_k, a->h_k, false},
                            {"v", a->v, a->v_batch_stride, a->v_row_stride, a->v_head_stride, nb_k, rows_k, a->h_k, false},
                            {"o", a->o, a->o_batch_stride, a->o_row_stride, a->o_head_stride, nb, rows_q, a->h, writes}});
}
int check_bwd_layout(const char* fn, const FaBwdParams* a, bool varlen, bool writes = true) {
  const int64_t nb = varlen ? 1 : a->b, rq = varlen ? a->total_q : a->seqlen_q, rk = varlen ? (a->total_k > 0 ? a->total_k : kMany) : a->seqlen_k;
  return check_layouts(fn, {{"dout", a->dout, a->do_batch_stride, a->do_row_stride, a->do_head_stride, nb, rq, a->h, false},
                            {"q", a->q, a->q_batch_stride, a->q_row_stride, a->q_head_stride, nb, rq, a->h, false},
                            {"k", a->k, a->k_batch_stride, a->k_row_stride, a->k_head_stride, nb, rk, a->h_k, false},
                            {"v", a->v, a->v_batch_stride, a->v_row_stride, a->v_head_stride, nb, rk, a->h_k, false},
                            {"o", a->o, a->o_batch_stride, a->o_row_stride, a->o_head_stride, nb, rq, a->h, false},
                            {"dq", a->dq, a->dq_batch_stride, a->dq_row_stride, a->dq_head_stride, nb, rq, a->h, writes},
                            {"dk", a->dk, a->dk_batch_stride, a->dk_row_stride, a->dk_head_stride, nb, rk, a->h_k, writes},
                            {"dv", a->dv, a->dv_batch_stride, a->dv_row_stride, a->dv_head_stride, nb, rk, a->h_k, writes}});
}

// A v / o head dim of its own (FaFwdParams::d_v / FaBwdParams::d_v; 0 = d).  One pair is built: q / k 192, v / o 128 (fa_fwd_dv.hip; the backward runs the
// 256-pitch kernels of head dim 192 with a value width of 128, fa_bwd.hip).  Everything else about such a call is refused here, before anything touches the
// device, with a message that names both head dims or the argument.
// (what neither built pair supports; `leftpad` = the argument's name in the entry point's words)
int refuse_pair_features(const char* fn, int d, int d_v, float p_dropout, float softcap, const void* alibi, const void* randval, const void* block_table,
                         const void* leftpad_k, const char* leftpad) {
  if (p_dropout > 0.f) return fail(FA_ERR_UNSUPPORTED, "%s: head dims (%d, %d) do not support dropout (p_dropout)", fn, d, d_v);
  if (softcap > 0.f) return fail(FA_ERR_UNSUPPORTED, "%s: head dims (%d, %d) do not support softcap", fn, d, d_v);
  if (alibi) return fail(FA_ERR_UNSUPPORTED, "%s: head dims (%d, %d) do not support ALiBi (alibi_slopes)", fn, d, d_v);
  if (randval) return fail(FA_ERR_UNSUPPORTED, "%s: head dims (%d, %d) do not support return_softmax", fn, d, d_v);
  if (block_table) return fail(FA_ERR_UNSUPPORTED, "%s: head dims (%d, %d) do not support block_table (paged KV)", fn, d, d_v);
  if (leftpad_k) return fail(FA_ERR_UNSUPPORTED, "%s: head dims (%d, %d) do not support %s", fn, d, d_v, leftpad);
  return FA_OK;
}
int check_value_dim(const char* fn, int d, int d_v, float p_dropout, float softcap, const void* alibi, const void* randval, const void* block_table,
                    const void* leftpad_k, bool kvcache, bool fp8, bool kvcache_entry = false) {
  if (d_v < 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: d_v must be non-negative (0 = the head dim of q / k), got %d", fn, d_v);
  if (d_v == 0 || d_v == d) return FA_OK;
  if (fp8) return fail(FA_ERR_UNSUPPORTED, "%s: head dims (%d, %d): the fp8 path has no kernel for a v head dim that differs from q / k", fn, d, d_v);
  if (mla_pair(d, d_v)) {   // the absorbed MLA decode shape: fa_fwd_kvcache alone (fa_fwd_mla.hip), plain attention under causal / window masks
    if (!kvcache_entry)
      return fail(FA_ERR_UNSUPPORTED, "%s: head dims (%d, %d): the absorbed MLA decode pair is built for fa_fwd_kvcache only (no fa_fwd / fa_varlen_fwd, no backward)", fn, d, d_v);
    return refuse_pair_features(fn, d, d_v, p_dropout, softcap, alibi, randval, nullptr, leftpad_k, "leftpad_k (cache_leftpad)");
  }
  if (kvcache) return fail(FA_ERR_UNSUPPORTED, "%s: head dims (%d, %d): the KV-cache path has no kernel for a v head dim that differs from q / k", fn, d, d_v);
  if (d != 192 || d_v != 128)
    return fail(FA_ERR_UNSUPPORTED, "%s: head dims (%d, %d): the only built pair with a v head dim that differs from q / k is (192, 128)", fn, d, d_v);
  return refuse_pair_features(fn, d, d_v, p_dropout, softcap, alibi, randval, block_table, leftpad_k, "leftpad_k");
}

// The device-side parameter block of a forward call, from (params, plan); every forward entry point fills it here.  (What an entry point refuses -- the fp8 paths take
// no ALiBi, softcap, dropout, left padding ... -- is NULL / 0 in a call that got this far.)  A forced num_splits > 1 that the workspace cannot hold is refused here.
int fill_fwd_k(const char* fn, const FaFwdParams* a, const FwdPlan& pl, fa::FwdK& k) {
  k = fa::FwdK{};
  k.n_splits = 1;
  k.pack_g = 1;
  k.q = a->q; k.k = a->k; k.v = a->v; k.o = a->o; k.lse = a->softmax_lse;
  k.q_bs = a->q_batch_stride; k.q_rs = a->q_row_stride; k.q_hs = a->q_head_stride;
  k.k_bs = a->k_batch_stride; k.k_rs = a->k_row_stride; k.k_hs = a->k_head_stride;
  k.v_bs = a->v_batch_stride; k.v_rs = a->v_row_stride; k.v_hs = a->v_head_stride;
  k.o_bs = a->o_batch_stride; k.o_rs = a->o_row_stride; k.o_hs = a->o_head_stride;
  k.cu_q = a->cu_seqlens_q; k.cu_k = a->cu_seqlens_k; k.seqused_k = a->seqused_k; k.seqused_q = a->seqused_q;
  k.kv_batch_idx = a->cache_batch_idx; k.block_table = a->block_table; k.block_table_bs = a->block_table_batch_stride;
  k.page_size = a->page_block_size; k.seqused_add = a->seqused_k_add; k.leftpad_k = a->leftpad_k;
  k.alibi = a->alibi_slopes; k.alibi_bs = a->alibi_batch_stride;
  k.b = a->b; k.h = a->h; k.h_k = a->h_k; k.hk_ratio = a->h / a->h_k;
  k.sq = a->seqlen_q; k.sk = a->seqlen_k; k.total_q = a->total_q;
  k.wl = pl.wl; k.wr = pl.wr;
  k.scale = a->softmax_scale;
  k.scale_log2 = a->softmax_scale * 1.4426950408889634f;
  k.softcap = a->softcap;
  fill_dropout(k, a->p_dropout, a->rng_state);
  if (a->p_dropout > 0.f) { k.randval = a->randval; k.rv_bs = a->randval_batch_stride; k.rv_hs = a->randval_head_stride; k.rv_rs = a->randval_row_stride; }
  // Deferred O rescale: the running max only moves when a row's max grew by more than this many log2
  // units (P stays <= 2^thr; fp32 accumulators and the relative precision of bf16/fp16 P are unaffected).
  // 0 reproduces the reference's rescale-on-any-growth rule exactly.  Default 8 (measured +4..10 %,
  // parity suite unchanged); override with FA_RESCALE_THR.
  // fp16 P must stay below 65504: the threshold is capped at 15 there (bf16 has fp32's exponent range).
  k.rescale_thr = fa::knobs().rescale_thr;
  if (a->dtype == FA_DTYPE_FP16 && k.rescale_thr > 15.f) k.rescale_thr = 15.f;
  // P is rounded to e4m3 (largest finite value 448): the deferred rescale may let it grow to 2^thr, so thr <= 8 (P <= 256)
  if (a->dtype == FA_DTYPE_FP8_E4M3) k.rescale_thr = std::min(k.rescale_thr, 8.f);
  if (pl.pack > 1) { k.pack_g = pl.pack; k.h = a->h_k; k.hk_ratio = 1; k.sq = a->seqlen_q * pl.pack; }   // grouped query heads become rows of one block
  if (pl.bounded) k.d_chunks = a->d / 8;
  if (pl.n_splits > 1) {   // the split the workspace grants: partial O rows of the plan's pitch, then the partial LSEs
    k.n_splits = pl.n_splits; k.split_tiles = pl.split_tiles;
    k.o_accum = (float*)a->workspace;
    k.lse_accum = k.o_accum + (int64_t)pl.n_splits * a->b * a->h * a->seqlen_q * pl.split_pitch;
  } else if (pl.want_splits > 1 && a->num_splits > 1) {
    return fail(FA_ERR_WORKSPACE, "%s: num_splits = %d needs a workspace of %lld bytes (fa_fwd_workspace_bytes)", fn, a->num_splits, (long long)pl.split_bytes);
  }  // auto schedule without a workspace: run unsplit
  k.nmb = (k.sq + pl.bm - 1) / pl.bm;
  fa::choose_units(a->b, a->h_k, k.hk_ratio, k.nmb * k.n_splits, k.n_units, k.unit_size, k.unit_hpx);
  return FA_OK;
}
inline int64_t workspace_on_offer(const void* workspace, int64_t bytes) { return workspace ? bytes : 0; }

int do_fwd(const FaFwdParams* a, void* stream, bool varlen, bool kvcache = false) {
  fa::launch_log_clear();
  if (!a) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
  g_err[0] = 0;
  if (int rc = check_common(a->b, a->h, a->h_k, a->d, a->dtype, a->softcap, a->d_v)) return rc;
  const char* fn = kvcache ? "fa_fwd_kvcache" : varlen ? "fa_varlen_fwd" : "fa_fwd";
  if (int rc = check_value_dim(fn, a->d, a->d_v, a->p_dropout, a->softcap, a->alibi_slopes, a->randval,
                               a->block_table, a->leftpad_k, kvcache || a->cache_batch_idx || a->seqused_k_add || a->num_splits > 1, false, kvcache)) return rc;
  const bool mla = kvcache && mla_pair(a->d, a->d_v);
  if (mla) {
    // V is the latent part of the same memory: the kernel reads every cache row once and uses it for both products (FwdK::v is never dereferenced)
    if (a->v != a->k || a->v_batch_stride != a->k_batch_stride || a->v_row_stride != a->k_row_stride || a->v_head_stride != a->k_head_stride)
      return fail(FA_ERR_UNSUPPORTED, "fa_fwd_kvcache: head dims (576, 512): V must be the first 512 channels of K (v == k with equal batch / row / head strides, "
                                      "i.e. the view k_cache[..., :512]); a separate V tensor is not supported");
    if (a->cu_seqlens_q || a->cu_seqlens_k || a->seqused_q)
      return fail(FA_ERR_UNSUPPORTED, "fa_fwd_kvcache: head dims (576, 512) do not support cu_seqlens_q / cu_seqlens_k / seqused_q");
    if (a->k_row_stride < 576 || a->q_row_stride % 8 || a->q_head_stride % 8 || a->q_batch_stride % 8 || a->k_row_stride % 8 || a->k_head_stride % 8 || a->k_batch_stride % 8 ||
        a->o_row_stride % 8 || a->o_head_stride % 8 || a->o_batch_stride % 8)
      return fail(FA_ERR_INVALID_ARGUMENT, "fa_fwd_kvcache: head dims (576, 512): q / k / o strides must be multiples of 8 elements and the k row stride at least 576");
    if ((((uintptr_t)a->q | (uintptr_t)a->k) & 15u) != 0 || ((uintptr_t)a->o & 7u) != 0)
      return fail(FA_ERR_INVALID_ARGUMENT, "fa_fwd_kvcache: head dims (576, 512): q and k must be 16-byte aligned, o 8-byte aligned");
  }
  if (!a->q || !a->k || !a->v || !a->o || !a->softmax_lse)
    return fail(FA_ERR_INVALID_ARGUMENT, "q, k, v, o and softmax_lse must be non-NULL");
  if (varlen != (a->cu_seqlens_q != nullptr) || varlen != (a->cu_seqlens_k != nullptr))
    return fail(FA_ERR_INVALID_ARGUMENT, varlen ? "fa_varlen_fwd needs cu_seqlens_q and cu_seqlens_k"
                                                : "fa_fwd takes fixed-length batches (cu_seqlens must be NULL)");
  if (a->seqlen_q < 0 || a->seqlen_k < 0) return fail(FA_ERR_INVALID_ARGUMENT, "negative sequence length");
  if (!kvcache && (a->cache_batch_idx || a->seqused_k_add))
    return fail(FA_ERR_INVALID_ARGUMENT, "cache_batch_idx / seqused_k_add are fa_fwd_kvcache arguments");
  if (!kvcache && !varlen && (a->block_table || a->leftpad_k))
    return fail(FA_ERR_INVALID_ARGUMENT, "block_table / leftpad_k are fa_varlen_fwd and fa_fwd_kvcache arguments");
  if (a->leftpad_k && a->block_table)
    return fail(FA_ERR_INVALID_ARGUMENT, "We don't support Paged KV and leftpad_k running at the same time yet");
  if (a->block_table) {
    if (a->cache_batch_idx) return fail(FA_ERR_INVALID_ARGUMENT, "Paged KVcache does not support cache_batch_idx");
    if (a->page_block_size <= 0 || a->page_block_size % 256 != 0)
      return fail(FA_ERR_INVALID_ARGUMENT, "Paged KV cache block size must be divisible by 256");
  }
  if (int rc = check_dropout(a->p_dropout, a->rng_state)) return rc;
  if (kvcache && a->p_dropout > 0.f) return fail(FA_ERR_INVALID_ARGUMENT, "fa_fwd_kvcache is an inference path: p_dropout must be 0");
  if (a->randval && !(a->p_dropout > 0.f)) return fail(FA_ERR_INVALID_ARGUMENT, "return_softmax is only supported when p_dropout > 0.0");
  if (a->num_splits > 1 && !kvcache) return fail(FA_ERR_INVALID_ARGUMENT, "num_splits > 1 is not supported");
  if (!mla) if (int rc = check_fwd_layout(fn, a, varlen, kvcache)) return rc;
  if (a->seqlen_q == 0 || a->total_q == 0) return FA_OK;  // nothing to write

  const FwdPlan pl = plan_fwd(a, kvcache ? kFaFwdKvcache : varlen ? kFaVarlenFwd : kFaFwd, workspace_on_offer(a->workspace, a->workspace_bytes));
  fa::FwdK k;
  if (int rc = fill_fwd_k(fn, a, pl, k)) return rc;
  if (int rc = fwd_work_list(a, pl, stream, k)) return rc;
  const int bf = a->dtype == FA_DTYPE_BF16;
  hipStream_t s = (hipStream_t)stream;
  const bool pair = pl.family == kFamMla || pl.family == kFamDv;
  int rc = pl.family == kFamMla       ? fa::launch_fwd_mla(k, bf, a->d, a->d_v, s)
           : pl.family == kFamDv      ? fa::launch_fwd_dv(k, bf, a->d, a->d_v, s)
           : pl.family == kFamW64     ? fa::launch_fwd_w64(k, bf, pl.dk, s)
           : pl.family == kFamPipelined ? fa::launch_fwd_il(k, bf, pl.dk, pl.schedule - 30, s)
                                      : fa::launch_fwd(k, bf, pl.dk, pl.schedule, s);
  if (rc == 0 && pl.family != kFamMla) { fa::last_schedule().fwd_pack = k.pack_g; if (!pair) fa::last_schedule().dv = fa::last_schedule().d; }
  if (rc == 0 && k.n_splits > 1) rc = fa::launch_splitkv_combine(k, bf, pl.family == kFamMla ? 512 : pl.dk, s);
  if (rc == -2) return pair ? fail(FA_ERR_UNSUPPORTED, "no forward kernel for head dims (%d, %d)", a->d, a->d_v) : fail(FA_ERR_UNSUPPORTED, "no forward kernel for head dim %d", a->d);
  if (rc == -3 && pl.family == kFamMla) return fail(FA_ERR_UNSUPPORTED, "k row stride too large: one 64-key tile (64 * row_stride * 2 bytes) must span less than 2 GiB");
  if (rc == -3 && pl.family != kFamDv)
    return fail(FA_ERR_UNSUPPORTED, pl.family == kFamW64 ? "k/v key range (or a 256-row q/o block) too large for the 64-rows-per-wave forward: (seqlen_k + 128) * k/v row_stride * 2 and 256 * q/o row_stride * 2 bytes must be < 4 GiB "
                                                           "(FA_FWD_NW=64 was forced; the default schedule falls back to the pipelined kernel)"
                                                         : "k/v row stride too large: one 64-key tile (64 * row_stride * 2 bytes) must span less than 2 GiB "
                                                           "(the kernels address a tile with 32-bit lane offsets)");
  if (rc != 0) return fail(FA_ERR_LAUNCH, "forward kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
  return FA_OK;
}

// Validates a backward call (check_bwd) and fills its device-side parameter block from (params, plan) (fill_bwd: also what the "does not apply after all"
// fallbacks of do_bwd start again from).
int check_bwd(const FaBwdParams* a, bool varlen) {
  if (!a) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
  g_err[0] = 0;
  if (int rc = check_common(a->b, a->h, a->h_k, a->d, a->dtype, a->softcap, a->d_v)) return rc;
  if (int rc = check_value_dim(varlen ? "fa_varlen_bwd" : "fa_bwd", a->d, a->d_v, a->p_dropout, a->softcap, a->alibi_slopes, nullptr, nullptr, nullptr, false, false)) return rc;
  if (!a->dout || !a->q || !a->k || !a->v || !a->o || !a->softmax_lse || !a->dq || !a->dk || !a->dv || !a->softmax_d)
    return fail(FA_ERR_INVALID_ARGUMENT, "dout, q, k, v, o, softmax_lse, dq, dk, dv and softmax_d must be non-NULL");
  if (varlen != (a->cu_seqlens_q != nullptr) || varlen != (a->cu_seqlens_k != nullptr))
    return fail(FA_ERR_INVALID_ARGUMENT, varlen ? "fa_varlen_bwd needs cu_seqlens_q and cu_seqlens_k"
                                                : "fa_bwd takes fixed-length batches (cu_seqlens must be NULL)");
  if (int rc = check_dropout(a->p_dropout, a->rng_state)) return rc;
  return check_bwd_layout(varlen ? "fa_varlen_bwd" : "fa_bwd", a, varlen);
}
void fill_bwd(const FaBwdParams* a, const BwdPlan& pl, fa::BwdK& k) {
  k = fa::BwdK{};
  k.dout = a->dout; k.q = a->q; k.k = a->k; k.v = a->v; k.o = a->o; k.lse = a->softmax_lse;
  k.dq = a->dq; k.dk = a->dk; k.dv = a->dv; k.delta = a->softmax_d;
  k.do_bs = a->do_batch_stride; k.do_rs = a->do_row_stride; k.do_hs = a->do_head_stride;
  k.q_bs = a->q_batch_stride; k.q_rs = a->q_row_stride; k.q_hs = a->q_head_stride;
  k.k_bs = a->k_batch_stride; k.k_rs = a->k_row_stride; k.k_hs = a->k_head_stride;
  k.v_bs = a->v_batch_stride; k.v_rs = a->v_row_stride; k.v_hs = a->v_head_stride;
  k.o_bs = a->o_batch_stride; k.o_rs = a->o_row_stride; k.o_hs = a->o_head_stride;
  k.dq_bs = a->dq_batch_stride; k.dq_rs = a->dq_row_stride; k.dq_hs = a->dq_head_stride;
  k.dk_bs = a->dk_batch_stride; k.dk_rs = a->dk_row_stride; k.dk_hs = a->dk_head_stride;
  k.dv_bs = a->dv_batch_stride; k.dv_rs = a->dv_row_stride; k.dv_hs = a->dv_head_stride;
  k.cu_q = a->cu_seqlens_q; k.cu_k = a->cu_seqlens_k; k.seqused_q = a->seqused_q; k.seqused_k = a->seqused_k;
  k.alibi = a->alibi_slopes; k.alibi_bs = a->alibi_batch_stride;
  k.b = a->b; k.h = a->h; k.h_k = a->h_k; k.hk_ratio = a->h / a->h_k;
  k.sq = a->seqlen_q; k.sk = a->seqlen_k; k.total_q = a->total_q; k.total_k = a->total_k;
  int causal = a->is_causal, wl = a->window_left, wr = a->window_right;
  normalize_window(a->seqlen_q, a->seqlen_k, a->alibi_slopes != nullptr, causal, wl, wr);
  k.wl = wl; k.wr = wr;
  k.scale = a->softmax_scale;
  k.scale_log2 = a->softmax_scale * 1.4426950408889634f;
  k.softcap = a->softcap;
  fill_dropout(k, a->p_dropout, a->rng_state);
  k.dq_nw = pl.dq_nw;
  if (!head_dim_native(a->d)) k.d_chunks = a->d / 8;   // run-time column bound of the next built size's kernels
  k.nmb = (a->seqlen_q + pl.bm - 1) / pl.bm;
  k.nnb = (a->seqlen_k + pl.bn - 1) / pl.bn;
  fa::choose_units(a->b, a->h_k, a->h / a->h_k, k.nmb, k.q_units, k.q_unit_size, k.q_unit_hpx);
  fa::choose_units(a->b, a->h_k, 1, k.nnb, k.k_units, k.k_unit_size, k.k_unit_hpx);
}

// the dK/dV launch of either schedule (-2 from the 64-keys-per-wave launcher = not covered after all: nothing was enqueued), on a split GQA group where the plan says so
int launch_dkdv_any(const FaBwdParams* a, const BwdPlan& pl, const fa::BwdK& k_in, int bf, int dk_, hipStream_t s) {
  fa::BwdK k = k_in;
  const GsplitPlan& gp = pl.gsplit;
  if (pl.split) {
    const int hk2 = a->h_k * gp.gs;
    k.h_k = hk2; k.hk_ratio = a->h / hk2; k.kv_in_shift = gp.shift;
    const int dvw = value_dim(a->d, a->d_v);
    k.dk = a->workspace; k.dv = (char*)a->workspace + gp.dk_bytes;
    k.dk_bs = (int64_t)a->seqlen_k * hk2 * a->d; k.dk_rs = (int64_t)hk2 * a->d; k.dk_hs = a->d;
    k.dv_bs = (int64_t)a->seqlen_k * hk2 * dvw; k.dv_rs = (int64_t)hk2 * dvw; k.dv_hs = dvw;
    fa::choose_units(a->b, hk2, 1, k.nnb, k.k_units, k.k_unit_size, k.k_unit_hpx);
  }
  int rc = -2, nw = 64;
  const bool own_dv = own_value_dim(a->d, a->d_v);
  if (pl.dkdv == 64) rc = fa::launch_bwd_dkdv_w64(k, bf, a->d, s);
  if (rc == -2) { nw = a->d > 128 ? 4 : 8; rc = own_dv ? fa::launch_bwd_dkdv_dv(k, bf, a->d, a->d_v, s) : fa::launch_bwd_dkdv(k, bf, dk_, s); }
  fa::last_schedule().bwd_dkdv_nw = nw;
  if (rc == 0 && pl.split) {
    rc = fa::launch_bwd_gsum(k.dk, k_in.dk, bf, a->b, a->seqlen_k, a->h_k, gp.gs, a->d, k_in.dk_bs, k_in.dk_rs, k_in.dk_hs, s);
    if (rc == 0) rc = fa::launch_bwd_gsum(k.dv, k_in.dv, bf, a->b, a->seqlen_k, a->h_k, gp.gs, value_dim(a->d, a->d_v), k_in.dv_bs, k_in.dv_rs, k_in.dv_hs, s);
  }
  return rc;
}

int do_bwd(const FaBwdParams* a, void* stream, bool varlen) {
  fa::launch_log_clear();
  if (int rc = check_bwd(a, varlen)) return rc;
  const BwdPlan pl = plan_bwd(a, workspace_on_offer(a->workspace, a->workspace_bytes));
  fa::BwdK k;
  fill_bwd(a, pl, k);
  hipStream_t s = (hipStream_t)stream;
  const int bf = a->dtype == FA_DTYPE_BF16;
  if (pl.kind == 5 && a->total_q != 0) {
    // delta pre-pass, then n_chunks + 1 mixed launches
    const C5Plan& c5 = pl.c5;
    k.nmb = c5.nmb; k.nnb = c5.nnb;
    k.k_units = a->b * a->h_k; k.k_unit_size = c5.nnb; k.k_unit_hpx = c5.hpx;
    k.ds_nq32 = c5.nq32; k.ds_nk32 = c5.pack.np64; k.ds_c1 = c5.pack.c1; k.ds_jb = c5.pack.jb; k.ds_head_tiles = c5.pack.head_tiles;
    k.c5_slot_bytes = (uint32_t)c5.slot_bytes;
    int rc = fa::launch_bwd_delta(k, bf, a->d, s);
    for (int c = 0; rc == 0 && c <= c5.n_chunks; ++c) {
      const int pj0 = c * c5.rounds_per_chunk, pj1 = std::min(c5.rounds, pj0 + c5.rounds_per_chunk);
      const int cj0 = (c - 1) * c5.rounds_per_chunk, cj1 = std::min(c5.rounds, cj0 + c5.rounds_per_chunk);
      k.ds_ws = (char*)a->workspace + (int64_t)(c & 1) * c5.slot_bytes;
      k.ds_rd = (const char*)a->workspace + (int64_t)((c + 1) & 1) * c5.slot_bytes;
      k.c5_np = c < c5.n_chunks ? 8 * (pj1 - pj0) * c5.nnb : 0;
      k.c5_nc = c >= 1 ? 8 * (cj1 - cj0) * (a->h / a->h_k) * c5.nmb : 0;
      k.c5_pbid0 = 8 * pj0 * c5.nnb; k.c5_pj0 = pj0; k.c5_cj0 = cj0;
      rc = fa::launch_bwd_c5(k, bf, a->d, s);
    }
    if (rc == 0) {
      fa::LastSchedule& ls = fa::last_schedule();
      ls.bwd_dkdv_nw = 64; ls.bwd_dq_nw = 64; ls.bwd_spill = 5; ls.bwd_list = 0;
      return FA_OK;
    }
    if (rc != -2) return fail(FA_ERR_LAUNCH, "backward kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    fill_bwd(a, pl, k);   // does not apply after all (nothing was enqueued but the delta pre-pass): the default path, from a clean parameter block
  }
  if (pl.kind == 3 && a->total_q != 0) {
    // delta pre-pass, then ONE launch: dK / dV and dQ = dS.K
    const FusedPlan& fpl = pl.fused;
    k.ds_ws = a->workspace;
    k.ds_nq32 = (a->seqlen_q + 31) / 32;
    k.ds_nk32 = (a->seqlen_k + 31) / 32;
    k.ds_np64 = fpl.pack.np64; k.ds_c1 = fpl.pack.c1; k.ds_jb = fpl.pack.jb; k.ds_head_tiles = fpl.pack.head_tiles;
    k.nmb = (a->seqlen_q + 255) / 256;
    k.fuse_sync = (int32_t*)((char*)a->workspace + fpl.ds_bytes);
    k.fuse_line = fa::knobs().fz_line;
    int rc = fa::launch_bwd_delta(k, bf, a->d, s);   // (the whole batch at once)
    const fa::BwdK whole = k;
    for (int b0 = 0; rc == 0 && b0 < a->b; b0 += fpl.nb) {   // one launch per chunk of batch entries, all on the same workspace
      const int nb = std::min(fpl.nb, a->b - b0);
      auto at = [&](const void* base, int64_t bs) { return (const void*)((const char*)base + (int64_t)b0 * bs * 2); };
      k = whole;
      k.b = nb;
      k.dout = at(whole.dout, whole.do_bs); k.q = at(whole.q, whole.q_bs); k.k = at(whole.k, whole.k_bs); k.v = at(whole.v, whole.v_bs); k.o = at(whole.o, whole.o_bs);
      k.dq = (void*)at(whole.dq, whole.dq_bs); k.dk = (void*)at(whole.dk, whole.dk_bs); k.dv = (void*)at(whole.dv, whole.dv_bs);
      k.lse = whole.lse + (int64_t)b0 * a->h * a->seqlen_q; k.delta = whole.delta + (int64_t)b0 * a->h * a->seqlen_q;
      fa::choose_units(nb, a->h_k, 1, k.nnb, k.k_units, k.k_unit_size, k.k_unit_hpx);
      k.fuse_items = nb * a->h * k.nmb;
      k.fuse_keep_err = b0 > 0;   // (the launch's error flag accumulates over the chunks: only the first launch zeroes it)
      rc = fa::launch_bwd_fused(k, bf, a->d, s);
    }
    k = whole;
    if (rc == 0) {
      fa::LastSchedule& ls = fa::last_schedule();
      ls.bwd_dkdv_nw = 8; ls.bwd_dq_nw = 8; ls.bwd_spill = 3; ls.bwd_list = 0;
      return FA_OK;
    }
    if (rc != -2) return fail(FA_ERR_LAUNCH, "backward kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    fill_bwd(a, pl, k);   // does not apply after all: the default path, from a clean parameter block
  }
  if (pl.lists) {   // (varlen only)
    const int64_t qe = pl.q_entries, ke = pl.k_entries;
    char* ws = (char*)a->workspace;
    fa::SchedK sk{};
    sk.nb = a->b; sk.wl = k.wl; sk.wr = k.wr;
    if (qe) {
      sk.cu_a = a->cu_seqlens_q; sk.cu_o = a->cu_seqlens_k; sk.list = (int2*)ws; sk.bound = (int)qe; sk.keys_blocked = 0;
      sk.blk = pl.bm;
      sk.work_shift = fa::sched_work_shift(a->seqlen_k);
      if (fa::launch_varlen_schedule(sk, s) != 0) return fail(FA_ERR_LAUNCH, "schedule kernel launch failed");
      k.q_list = (const int2*)ws; k.q_bound = (int)qe;
      ws += (qe + 1) * 8;
    }
    if (ke) {
      sk.cu_a = a->cu_seqlens_k; sk.cu_o = a->cu_seqlens_q; sk.list = (int2*)ws; sk.bound = (int)ke; sk.keys_blocked = 1;
      sk.blk = pl.bn;
      sk.work_shift = fa::sched_work_shift(a->seqlen_q);
      if (fa::launch_varlen_schedule(sk, s) != 0) return fail(FA_ERR_LAUNCH, "schedule kernel launch failed");
      k.k_list = (const int2*)ws; k.k_bound = (int)ke;
    }
  }
  // Nothing to differentiate: the caller's dq/dk/dv hold no rows (Sq == 0 / Sk == 0 with fixed
  // shapes are handled by the binder, which zero-fills as flash_api.cpp:992-999 does).
  if (a->seqlen_q == 0 || a->seqlen_k == 0 || a->total_q == 0 || a->total_k == 0) return FA_OK;
  const int dk_ = head_dim_kernel(a->d);   // kernel head dim (!= a->d: BwdK::d_chunks)
  // Round 4: where the 64-rows-per-wave dQ kernel runs (plain attention, head dim 64 / 128, long key loops) it computes softmax_d = rowsum(dO * O) of its own rows
  // in its prologue and goes FIRST; the dK/dV kernel behind it reads softmax_d from memory as before and the delta pre-pass is not launched
  // (FA_BWD_FUSE_DELTA=0: the three-launch order).  -2 from the launcher = the schedule does not apply after all: nothing was enqueued, fall through.
  if (k.dq_nw == 64 && fa::knobs().bwd_fuse_delta) {
    k.fuse_delta = 1;
    int rc = fa::launch_bwd_dq_w64(k, bf, a->d, s);
    if (rc == 0) {
      fa::last_schedule().bwd_dq_nw = 64;
      rc = launch_dkdv_any(a, pl, k, bf, dk_, s);
      fa::last_schedule().bwd_spill = 0; fa::last_schedule().bwd_list = (k.q_list != nullptr) + 2 * (k.k_list != nullptr);
      if (rc != 0) return fail(FA_ERR_LAUNCH, "backward kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
      return FA_OK;
    }
    if (rc != -2) return fail(FA_ERR_LAUNCH, "backward kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    k.fuse_delta = 0;
  }
  const bool own_dv = own_value_dim(a->d, a->d_v);   // q / k 192, v / o 128: the 256-pitch kernels with a value width of their own
  int rc = own_dv ? fa::launch_bwd_delta_dv(k, bf, a->d, a->d_v, s) : fa::launch_bwd_delta(k, bf, dk_, s);
  if (rc == 0) {
    rc = launch_dkdv_any(a, pl, k, bf, dk_, s);
  }
  if (rc == 0) rc = own_dv ? fa::launch_bwd_dq_dv(k, bf, a->d, a->d_v, s) : fa::launch_bwd_dq(k, bf, dk_, s);
  if (rc == 0) { fa::last_schedule().bwd_spill = 0; fa::last_schedule().bwd_list = (k.q_list != nullptr) + 2 * (k.k_list != nullptr); }
  if (rc == -2) return fail(FA_ERR_UNSUPPORTED, "no backward kernel for head dim %d", a->d);
  if (rc != 0) return fail(FA_ERR_LAUNCH, "backward kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
  return FA_OK;
}

// What both fp8 entry points check first, and refuse with the same words (`takes` = the entry point's tensors in its dtype message)
int check_fp8_args(const char* fn, const FaFwdParams* a, const char* takes) {
  if (a->dtype != FA_DTYPE_FP8_E4M3)
    return fail(FA_ERR_INVALID_ARGUMENT, "%s takes FA_DTYPE_FP8_E4M3 (float8_e4m3fn) %s, got dtype %d", fn, takes, a->dtype);
  if (a->b <= 0) return fail(FA_ERR_INVALID_ARGUMENT, "batch size must be positive");
  if (a->h <= 0 || a->h_k <= 0 || a->h % a->h_k != 0)
    return fail(FA_ERR_INVALID_ARGUMENT, "Number of heads in key/value must divide number of heads in query");
  if (int rc = check_value_dim(fn, a->d, a->d_v, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr, false, true)) return rc;
  if (a->d != 64 && a->d != 128) return fail(FA_ERR_UNSUPPORTED, "%s: head dim %d is not built (fp8 kernels: 64 and 128)", fn, a->d);
  if (a->softcap < 0.f) return fail(FA_ERR_INVALID_ARGUMENT, "softcap must be non-negative");
  if (a->softcap > 0.f) return fail(FA_ERR_UNSUPPORTED, "%s: softcap is not supported on the fp8 path", fn);
  if (a->alibi_slopes) return fail(FA_ERR_UNSUPPORTED, "%s: ALiBi is not supported on the fp8 path", fn);
  return FA_OK;
}
// 16-byte DMA pieces and stores: e4m3 rows start on 16 bytes, bf16 rows of o on 8 elements (a packed batch has no batch strides)
int check_fp8_layout(const char* fn, const FaFwdParams* a, bool varlen) {
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
  if (!al16(a->q) || !al16(a->k) || !al16(a->v) || !al16(a->o)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: q, k, v and o must be 16-byte aligned", fn);
  const int64_t in_strides[] = {a->q_row_stride, a->q_head_stride, a->k_row_stride, a->k_head_stride, a->v_row_stride, a->v_head_stride,
                                varlen ? 0 : a->q_batch_stride, varlen ? 0 : a->k_batch_stride, varlen ? 0 : a->v_batch_stride};
  for (int64_t s : in_strides)
    if (s % 16 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: q / k / v strides must be multiples of 16 bytes", fn);
  const int64_t o_strides[] = {a->o_row_stride, a->o_head_stride, varlen ? 0 : a->o_batch_stride};
  for (int64_t s : o_strides)
    if (s % 8 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: o (bf16) strides must be multiples of 8 elements", fn);
  return FA_OK;
}
// plan, fill, launch of a validated fp8 call (the partials of a split are fp32, o is bf16)
int run_fwd_fp8(const char* fn, const FaFwdParams* a, const FaFp8Params* f, FwdEntry e, void* stream) {
  const FwdPlan pl = plan_fwd(a, e, workspace_on_offer(a->workspace, a->workspace_bytes));
  fa::FwdK k;
  if (int rc = fill_fwd_k(fn, a, pl, k)) return rc;
  if (int rc = fwd_work_list(a, pl, stream, k)) return rc;
  fa::Fp8K f8{};
  if (f) {
    f8.q_descale = f->q_descale; f8.q_bs = f->q_descale_batch_stride; f8.q_hs = f->q_descale_head_stride;
    f8.k_descale = f->k_descale; f8.k_bs = f->k_descale_batch_stride; f8.k_hs = f->k_descale_head_stride;
    f8.v_descale = f->v_descale; f8.v_bs = f->v_descale_batch_stride; f8.v_hs = f->v_descale_head_stride;
  }
  int rc = pl.family == kFamFp8Kv ? fa::launch_fwd_fp8_kv(k, f8, a->d, (hipStream_t)stream) : fa::launch_fwd_fp8(k, f8, a->d, (hipStream_t)stream);
  if (rc == 0) fa::last_schedule().dv = a->d;
  if (rc == 0 && k.n_splits > 1) rc = fa::launch_splitkv_combine(k, 1, a->d, (hipStream_t)stream);
  if (rc == -2) return fail(FA_ERR_UNSUPPORTED, "%s: head dim %d is not built (fp8 kernels: 64 and 128)", fn, a->d);
  if (rc == -3) return fail(FA_ERR_UNSUPPORTED, "k/v row stride too large: one 64-key tile (64 * row_stride bytes) must span less than 2 GiB");
  if (rc != 0) return fail(FA_ERR_LAUNCH, "forward kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
  return FA_OK;
}

// FP8 forward (fa_fwd_fp8.hip): e4m3 q / k / v, bf16 o.  Plain attention under causal / window masks, head dims 64 / 128, fixed-length
// and packed batches; every other feature is refused here, before any launch.
int do_fwd_fp8(const FaFwdParams* a, const FaFp8Params* f, void* stream, bool varlen) {
  fa::launch_log_clear();
  if (!a) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
  g_err[0] = 0;
  const char* fn = varlen ? "fa_varlen_fwd_fp8" : "fa_fwd_fp8";
  if (int rc = check_fp8_args(fn, a, "q / k / v")) return rc;
  if (a->p_dropout != 0.f || a->rng_state) return fail(FA_ERR_UNSUPPORTED, "%s: dropout is not supported on the fp8 path", fn);
  if (a->randval) return fail(FA_ERR_UNSUPPORTED, "%s: return_softmax is not supported on the fp8 path", fn);
  if (a->seqused_q || a->seqused_k) return fail(FA_ERR_UNSUPPORTED, "%s: seqused_q / seqused_k are not supported on the fp8 path", fn);
  if (a->leftpad_k) return fail(FA_ERR_UNSUPPORTED, "%s: leftpad_k is not supported on the fp8 path", fn);
  if (a->block_table) return fail(FA_ERR_UNSUPPORTED, "%s: block_table (paged KV) is not supported on the fp8 path", fn);
  if (a->cache_batch_idx || a->seqused_k_add || a->num_splits > 1)
    return fail(FA_ERR_UNSUPPORTED, "%s: the KV-cache arguments (cache_batch_idx, seqused_k_add, num_splits) have no fp8 path", fn);
  if (!a->q || !a->k || !a->v || !a->o || !a->softmax_lse)
    return fail(FA_ERR_INVALID_ARGUMENT, "q, k, v, o and softmax_lse must be non-NULL");
  if (varlen != (a->cu_seqlens_q != nullptr) || varlen != (a->cu_seqlens_k != nullptr))
    return fail(FA_ERR_INVALID_ARGUMENT, varlen ? "fa_varlen_fwd_fp8 needs cu_seqlens_q and cu_seqlens_k"
                                                : "fa_fwd_fp8 takes fixed-length batches (cu_seqlens must be NULL)");
  if (a->seqlen_q < 0 || a->seqlen_k < 0) return fail(FA_ERR_INVALID_ARGUMENT, "negative sequence length");
  if (int rc = check_fp8_layout(fn, a, varlen)) return rc;
  if (a->seqlen_q == 0 || a->total_q == 0) return FA_OK;  // nothing to write
  return run_fwd_fp8(fn, a, f, varlen ? kFaVarlenFwdFp8 : kFaFwdFp8, stream);
}

// FP8 forward against an fp8 KV cache (fa_fwd_fp8_kv.hip): the decode side of do_fwd_fp8.  cache_seqlens (seqused_k + seqused_k_add), cache_batch_idx, a paged
// cache, causal / window masks, head packing and split keys as fa_fwd_kvcache; everything else is refused here, before any launch.
int do_fwd_kvcache_fp8(const FaFwdParams* a, const FaFp8Params* f, void* stream) {
  fa::launch_log_clear();
  if (!a) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
  g_err[0] = 0;
  const char* fn = "fa_fwd_kvcache_fp8";
  if (int rc = check_fp8_args(fn, a, "q and k / v caches")) return rc;
  if (a->p_dropout != 0.f || a->rng_state || a->randval) return fail(FA_ERR_UNSUPPORTED, "%s: dropout / return_softmax are not supported on the fp8 path", fn);
  if (a->leftpad_k) return fail(FA_ERR_UNSUPPORTED, "%s: leftpad_k (cache_leftpad) is not supported on the fp8 path", fn);
  if (a->seqused_q) return fail(FA_ERR_UNSUPPORTED, "%s: seqused_q is not supported on the fp8 path", fn);
  if (a->cu_seqlens_q || a->cu_seqlens_k) return fail(FA_ERR_INVALID_ARGUMENT, "%s takes fixed-length batches (cu_seqlens must be NULL)", fn);
  if (!a->q || !a->k || !a->v || !a->o || !a->softmax_lse)
    return fail(FA_ERR_INVALID_ARGUMENT, "q, k, v, o and softmax_lse must be non-NULL");
  if (a->seqlen_q < 0 || a->seqlen_k < 0 || a->seqused_k_add < 0) return fail(FA_ERR_INVALID_ARGUMENT, "negative sequence length");
  if (a->num_splits < 0) return fail(FA_ERR_INVALID_ARGUMENT, "num_splits must be >= 0");
  if (a->block_table) {
    if (a->cache_batch_idx) return fail(FA_ERR_INVALID_ARGUMENT, "Paged KVcache does not support cache_batch_idx");
    if (a->page_block_size <= 0 || a->page_block_size % 256 != 0)
      return fail(FA_ERR_INVALID_ARGUMENT, "Paged KV cache block size must be divisible by 256");
    if (a->seqlen_k <= 0 || a->seqlen_k % a->page_block_size != 0)
      return fail(FA_ERR_INVALID_ARGUMENT, "%s: with block_table, seqlen_k is max_num_blocks_per_seq * page_block_size (at least one page)", fn);
  }
  if (int rc = check_fp8_layout(fn, a, false)) return rc;
  if (a->seqlen_q == 0 || a->total_q == 0) return FA_OK;  // nothing to write
  return run_fwd_fp8(fn, a, f, kFaFwdKvcacheFp8, stream);
}

}  // namespace

extern "C" {

int fa_abi_version(void) { return FA_ABI_VERSION; }
int fa_sizeof_fp8_params(void) { return (int)sizeof(FaFp8Params); }
int fa_fwd_fp8(const FaFwdParams* params, const FaFp8Params* fp8, void* stream) { return do_fwd_fp8(params, fp8, stream, false); }
int fa_varlen_fwd_fp8(const FaFwdParams* params, const FaFp8Params* fp8, void* stream) { return do_fwd_fp8(params, fp8, stream, true); }
int fa_fwd_kvcache_fp8(const FaFwdParams* params, const FaFp8Params* fp8, void* stream) { return do_fwd_kvcache_fp8(params, fp8, stream); }
int fa_sizeof_fwd_params(void) { return (int)sizeof(FaFwdParams); }
int fa_sizeof_bwd_params(void) { return (int)sizeof(FaBwdParams); }
int fa_sizeof_kvappend_params(void) { return (int)sizeof(FaKvAppendParams); }
int fa_sizeof_rotary_params(void) { return (int)sizeof(FaRotaryParams); }
const char* fa_last_error(void) { return g_err; }
void fa_knobs_reload(void) { g_knobs.store(read_knobs(), std::memory_order_release); }
int fa_last_schedule(int32_t* out, int n) {
  const fa::LastSchedule& ls = fa::last_schedule();
  const int32_t v[FA_SCHEDULE_FIELDS] = {ls.fwd_kernel, ls.fwd_nw, ls.fwd_feat, ls.fwd_splits, ls.fwd_list, ls.d, ls.bf16, ls.bwd_dq_nw, ls.bwd_list, ls.bwd_spill, ls.fwd_pack, ls.bwd_dkdv_nw, ls.dv};
  for (int i = 0; i < n && i < FA_SCHEDULE_FIELDS; ++i) out[i] = v[i];
  return FA_SCHEDULE_FIELDS;
}
const char* fa_last_kernel_name(void) { return fa::last_schedule().name; }
// The kernels of the calling thread's last launching call, as the symbol names of the code objects, one per line.  A kernel's host-side handle carries the
// device symbol's name in the library's dynamic symbol table (dladdr: host only, works before any device is touched); a handle that is not exported is asked of
// the runtime (hipKernelNameRefByPtr); "?" if neither knows it.
int fa_launch_log(char* buf, int n) {
  const int count = fa::launch_log_count();
  int used = 0;   // bytes of text so far, without the terminator
  if (buf && n > 0) buf[0] = 0;
  for (int i = 0; i < count; ++i) {
    const void* kern = fa::launch_log_at(i);
    const char* name = nullptr;
    Dl_info info;
    if (kern && dladdr(kern, &info) != 0 && info.dli_sname && info.dli_saddr == kern) name = info.dli_sname;
    if (kern && !name) name = hipKernelNameRefByPtr(kern, nullptr);
    if (!name || !*name) name = kern ? "?" : "?overflow";
    const int len = (int)strlen(name);
    if (buf && used + len + 1 < n) { memcpy(buf + used, name, len); buf[used + len] = '\n'; buf[used + len + 1] = 0; }
    used += len + 1;
  }
  return used + 1;
}
// (the plan of the entry points without a KV cache: no split keys)
int fa_fwd_schedule_query(const FaFwdParams* a, int varlen) {
  if (!a) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
  if (int rc = check_common(a->b, a->h, a->h_k, a->d, a->dtype, a->softcap, a->d_v)) return rc;
  if (int rc = check_value_dim("fa_fwd_schedule_query", a->d, a->d_v, a->p_dropout, a->softcap, a->alibi_slopes, a->randval, a->block_table, a->leftpad_k,
                               a->cache_batch_idx || a->seqused_k_add || a->num_splits > 1, false)) return rc;   // (the MLA decode pair too: fa_fwd_kvcache only)
  if (int rc = check_fwd_layout("fa_fwd_schedule_query", a, varlen != 0, false, false)) return rc;
  return plan_fwd(a, varlen ? kFaVarlenFwd : kFaFwd, kAnyWorkspace).schedule;
}
int fa_bwd_dq_schedule_query(const FaBwdParams* a) {
  if (!a) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
  if (int rc = check_common(a->b, a->h, a->h_k, a->d, a->dtype, a->softcap, a->d_v)) return rc;
  if (int rc = check_value_dim("fa_bwd_dq_schedule_query", a->d, a->d_v, a->p_dropout, a->softcap, a->alibi_slopes, nullptr, nullptr, nullptr, false, false)) return rc;
  if (int rc = check_bwd_layout("fa_bwd_dq_schedule_query", a, a->cu_seqlens_q != nullptr, false)) return rc;
  return plan_bwd(a, kAnyWorkspace).dq_nw;
}

int fa_bwd_plan_query(const FaBwdParams* a, int32_t* out, int n) {
  if (!a || !out) return fail(FA_ERR_INVALID_ARGUMENT, "params / out is NULL");
  if (int rc = check_common(a->b, a->h, a->h_k, a->d, a->dtype, a->softcap)) return rc;
  if (int rc = check_bwd_layout("fa_bwd_plan_query", a, a->cu_seqlens_q != nullptr, false)) return rc;
  int32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const BwdPlan pl = plan_bwd(a, kAnyWorkspace);
  v[0] = pl.kind;
  if (pl.kind == 5) {
    v[1] = pl.c5.n_chunks; v[2] = pl.c5.rounds_per_chunk; v[3] = pl.c5.pack.head_tiles; v[4] = pl.c5.pack.np64; v[5] = pl.c5.pack.c1; v[6] = pl.c5.pack.jb; v[7] = (int32_t)(pl.c5.slot_bytes >> 20);
  } else if (pl.kind == 3) {
    v[1] = pl.fused.n_chunks; v[2] = pl.fused.nb; v[7] = (int32_t)(pl.ws_bytes >> 20);
  } else if (pl.split) {   // (the pair: its dK/dV half on a split GQA group)
    v[3] = pl.gsplit.gs; v[7] = (int32_t)(pl.gsplit.bytes >> 20);
  }
  for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
  return 8;
}

int fa_fwd(const FaFwdParams* params, void* stream) { return do_fwd(params, stream, false); }
int fa_varlen_fwd(const FaFwdParams* params, void* stream) { return do_fwd(params, stream, true); }
int fa_fwd_kvcache(const FaFwdParams* params, void* stream) { return do_fwd(params, stream, false, true); }

int fa_kvcache_append(const FaKvAppendParams* a, void* stream) {
  fa::launch_log_clear();
  if (!a) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
  g_err[0] = 0;
  if (!a->knew || !a->vnew || !a->kcache || !a->vcache) return fail(FA_ERR_INVALID_ARGUMENT, "knew, vnew, kcache and vcache must be non-NULL");
  const bool fp8 = a->dtype == FA_DTYPE_FP8_E4M3;   // one byte per element: the copy kernel moves 16-byte chunks of 16-bit words, so the row is d / 2 words
  if (a->d <= 0 || a->d % (fp8 ? 16 : 8) != 0) return fail(FA_ERR_INVALID_ARGUMENT, fp8 ? "fa_kvcache_append: the head dimension of an e4m3 cache must be a multiple of 16" : "head dimension must be a multiple of 8");
  if (a->dtype != FA_DTYPE_FP16 && a->dtype != FA_DTYPE_BF16 && !fp8) return fail(FA_ERR_INVALID_ARGUMENT, "FlashAttention only supports fp16 and bf16 data type");
  if (a->block_table && (a->page_block_size <= 0 || a->page_block_size % 256 != 0))
    return fail(FA_ERR_INVALID_ARGUMENT, "Paged KV cache block size must be divisible by 256");
  if (fp8) {
    if (a->block_table && a->cache_batch_idx) return fail(FA_ERR_INVALID_ARGUMENT, "Paged KVcache does not support cache_batch_idx");
    if ((((uintptr_t)a->knew | (uintptr_t)a->vnew | (uintptr_t)a->kcache | (uintptr_t)a->vcache) & 15u) != 0)
      return fail(FA_ERR_INVALID_ARGUMENT, "fa_kvcache_append: e4m3 knew, vnew, kcache and vcache must be 16-byte aligned");
    const int64_t strides[] = {a->knew_batch_stride, a->knew_row_stride, a->knew_head_stride, a->vnew_batch_stride, a->vnew_row_stride, a->vnew_head_stride,
                               a->kcache_batch_stride, a->kcache_row_stride, a->kcache_head_stride, a->vcache_batch_stride, a->vcache_row_stride, a->vcache_head_stride};
    for (int64_t st : strides)
      if (st % 16 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "fa_kvcache_append: e4m3 strides must be multiples of 16 bytes");
  }
  if (!fp8)
    if (int rc = check_layouts("fa_kvcache_append", {{"knew", a->knew, a->knew_batch_stride, a->knew_row_stride, a->knew_head_stride, a->b, a->seqlen_new, a->h_k, false},
                                                     {"vnew", a->vnew, a->vnew_batch_stride, a->vnew_row_stride, a->vnew_head_stride, a->b, a->seqlen_new, a->h_k, false},
                                                     {"kcache", a->kcache, a->kcache_batch_stride, a->kcache_row_stride, a->kcache_head_stride, kMany, kMany, a->h_k, true},
                                                     {"vcache", a->vcache, a->vcache_batch_stride, a->vcache_row_stride, a->vcache_head_stride, kMany, kMany, a->h_k, true}})) return rc;
  fa::KvAppendK k{};
  k.knew = a->knew; k.vnew = a->vnew; k.kcache = a->kcache; k.vcache = a->vcache;
  k.kn_bs = a->knew_batch_stride; k.kn_rs = a->knew_row_stride; k.kn_hs = a->knew_head_stride;
  k.vn_bs = a->vnew_batch_stride; k.vn_rs = a->vnew_row_stride; k.vn_hs = a->vnew_head_stride;
  k.kc_bs = a->kcache_batch_stride; k.kc_rs = a->kcache_row_stride; k.kc_hs = a->kcache_head_stride;
  k.vc_bs = a->vcache_batch_stride; k.vc_rs = a->vcache_row_stride; k.vc_hs = a->vcache_head_stride;
  k.seqlens_k = a->seqlens_k; k.kv_batch_idx = a->cache_batch_idx; k.block_table = a->block_table;
  k.block_table_bs = a->block_table_batch_stride; k.page_size = a->page_block_size;
  k.b = a->b; k.s_new = a->seqlen_new; k.h_k = a->h_k; k.d = a->d;
  // V is a view of the K rows on both sides (e.g. the absorbed MLA cache: v = k[..., :512]; any dtype, any d): the key copy already writes every byte, once
  if (a->vnew == a->knew && a->vcache == a->kcache && k.vn_bs == k.kn_bs && k.vn_rs == k.kn_rs && k.vn_hs == k.kn_hs && k.vc_bs == k.kc_bs && k.vc_rs == k.kc_rs && k.vc_hs == k.kc_hs)
    k.vnew = nullptr;
  if (fp8) {   // bytes -> 16-bit words (a byte copy: nothing is requantised)
    k.d /= 2;
    for (int64_t* st : {&k.kn_bs, &k.kn_rs, &k.kn_hs, &k.vn_bs, &k.vn_rs, &k.vn_hs, &k.kc_bs, &k.kc_rs, &k.kc_hs, &k.vc_bs, &k.vc_rs, &k.vc_hs}) *st /= 2;
  }
  if (fa::launch_kv_append(k, (hipStream_t)stream) != 0)
    return fail(FA_ERR_LAUNCH, "kv append launch failed: %s", hipGetErrorString(hipGetLastError()));
  return FA_OK;
}

int fa_rotary(const FaRotaryParams* a, void* stream) {
  fa::launch_log_clear();
  if (!a) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
  g_err[0] = 0;
  if (!a->x || !a->y || !a->cos || !a->sin) return fail(FA_ERR_INVALID_ARGUMENT, "x, y, cos and sin must be non-NULL");
  if (a->dtype == FA_DTYPE_FP8_E4M3) return fail(FA_ERR_UNSUPPORTED, "fa_rotary: rotary on float8_e4m3fn values needs a requantisation that is not defined (rotate before quantising)");
  if (a->dtype != FA_DTYPE_FP16 && a->dtype != FA_DTYPE_BF16) return fail(FA_ERR_INVALID_ARGUMENT, "FlashAttention only supports fp16 and bf16 data type");
  if (a->d <= 0 || a->d % 8 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "head dimension must be a multiple of 8");
  if (a->rotary_dim <= 0 || a->rotary_dim > a->d) return fail(FA_ERR_INVALID_ARGUMENT, "rotary_dim must be <= headdim");
  if (a->rotary_dim % 16 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "Only rotary dimensions divisible by 16 are currently supported");
  if (a->seqlen_ro <= 0) return fail(FA_ERR_INVALID_ARGUMENT, "cos/sin must have at least one row");
  if (int rc = check_layouts("fa_rotary", {{"x", a->x, a->x_batch_stride, a->x_row_stride, a->x_head_stride, a->b, a->s, a->h, false},
                                           {"y", a->y, a->y_batch_stride, a->y_row_stride, a->y_head_stride, a->b, a->s, a->h, true}})) return rc;
  fa::RotaryK k{};
  k.x = a->x; k.y = a->y; k.cos = a->cos; k.sin = a->sin; k.offsets = a->seqlen_offsets;
  k.x_bs = a->x_batch_stride; k.x_rs = a->x_row_stride; k.x_hs = a->x_head_stride;
  k.y_bs = a->y_batch_stride; k.y_rs = a->y_row_stride; k.y_hs = a->y_head_stride; k.cos_rs = a->cos_row_stride;
  k.b = a->b; k.s = a->s; k.h = a->h; k.d = a->d; k.rotary_dim = a->rotary_dim; k.seqlen_ro = a->seqlen_ro;
  k.interleaved = a->interleaved; k.per_token = a->per_token;
  if (fa::launch_rotary(k, a->dtype == FA_DTYPE_BF16, (hipStream_t)stream) != 0)
    return fail(FA_ERR_LAUNCH, "rotary launch failed: %s", hipGetErrorString(hipGetLastError()));
  return FA_OK;
}

int fa_set_rng_state(uint64_t seed, uint64_t offset, uint64_t* rng_state, void* stream) {
  fa::launch_log_clear();
  g_err[0] = 0;
  if (!rng_state) return fail(FA_ERR_INVALID_ARGUMENT, "rng_state is NULL");
  if (fa::launch_set_rng(seed, offset, rng_state, (hipStream_t)stream) != 0)
    return fail(FA_ERR_LAUNCH, "rng_state launch failed: %s", hipGetErrorString(hipGetLastError()));
  return FA_OK;
}

int64_t fa_fwd_workspace_bytes(const FaFwdParams* params) {
  if (!params) return 0;
  // (a layout the launching call refuses gets no workspace: the refusal, with its message, comes from that call)
  if (params->dtype != FA_DTYPE_FP8_E4M3 && !mla_pair(params->d, params->d_v) &&
      check_fwd_layout("fa_fwd_workspace_bytes", params, params->cu_seqlens_q != nullptr, !params->cu_seqlens_q, false) != FA_OK) return 0;
  // (no entry argument: a packed batch is fa_varlen_fwd's or fa_varlen_fwd_fp8's -- the work list of an uneven batch --, any fixed-length call counts as a KV-cache
  // call -- the partial rows of split keys)
  const bool fp8 = params->dtype == FA_DTYPE_FP8_E4M3;
  const FwdEntry e = params->cu_seqlens_q ? (fp8 ? kFaVarlenFwdFp8 : kFaVarlenFwd) : (fp8 ? kFaFwdKvcacheFp8 : kFaFwdKvcache);
  return plan_fwd(params, e, kAnyWorkspace, true).ws_bytes;
}

int64_t fa_bwd_workspace_bytes(const FaBwdParams* params) {
  // no fp32 dq accumulator; an uneven packed batch gets work lists, a fixed-length batch the dS workspace of the 5-contraction path
  if (!params) return 0;
  if (check_bwd_layout("fa_bwd_workspace_bytes", params, params->cu_seqlens_q != nullptr, false) != FA_OK) return 0;   // (as fa_fwd_workspace_bytes)
  return plan_bwd(params, kAnyWorkspace, true).ws_bytes;
}
int fa_bwd(const FaBwdParams* params, void* stream) { return do_bwd(params, stream, false); }
int fa_bwd_fused_status(const FaBwdParams* params, void* stream) {
  if (!params || !params->workspace || fa::last_schedule().bwd_spill != 3) return FA_OK;   // (this thread's last backward did not take the fused path: the sync area was never initialised)
  // Reading the flag synchronises the stream.  Where the fused backward is the DEFAULT (round 6: the table of bwd_fused_by_table) the binders' call returns at once --
  // a host sync per backward is not acceptable there, and the flag guards a wait that cannot time out while the launch's workgroups run (the publisher a consumer
  // polls for is between two of its own instructions); FA_BWD_MODE=3 (the opt-in form) and FA_BWD_FUSED_CHECK=1 read it.
  if (fa::knobs().bwd_fused_check < 0 || (fa::knobs().bwd_mode != 3 && !fa::knobs().bwd_fused_check)) return FA_OK;   // (-1: never, also for FA_BWD_MODE=3 -- timing the launch without the sync)
  const BwdPlan pl = plan_bwd(params, params->workspace_bytes);
  if (pl.kind != 3) return FA_OK;   // the call did not (could not) take the fused path
  const int64_t fz = pl.fused.ds_bytes;
  int32_t flag = 0;
  if (hipMemcpyAsync(&flag, (const char*)params->workspace + fz + fa::FZ_ERR * 4, sizeof(flag), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return fail(FA_ERR_LAUNCH, "fused backward: could not read the launch's error flag: %s", hipGetErrorString(hipGetLastError()));
  if (flag != 0) return fail(FA_ERR_LAUNCH, "fused backward (FA_BWD_MODE=3): a dQ hand-off timed out, a block of dq was not written -- discard this call's gradients");
  return FA_OK;
}
int fa_varlen_bwd(const FaBwdParams* params, void* stream) { return do_bwd(params, stream, true); }

}  // extern "C"
