// What a C-ABI call will run, decided ONCE: plan_fwd / plan_bwd turn (parameters, entry point, workspace on offer) into a plain struct -- kernel family, schedule,
// block rows, head packing, key splits, work lists, workspace bytes -- that the launching functions of fa_api.cpp execute and the queries (fa_fwd_schedule_query,
// fa_fwd_workspace_bytes, fa_bwd_plan_query, ...) report, the latter with as much workspace on offer as the plan asks for.  Nothing here calls the HIP runtime or
// launches anything.  Included by fa_api.cpp alone (internal linkage throughout); the parameters are taken as validated by the caller where a launch follows.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/fa_gfx950.h"
#include "fa_device.h"
#include "fa_kernel_params.h"
#include "fa_launch.h"

namespace {

// Head dims with their own kernels (the reference builds the same set: static_switch.h:92-110).  32 / 96 / 192 are "trimmed"
// variants of the 64 / 128 / 256 kernels (fa_fwd.hip: same LDS pitch, fewer k-steps and output blocks) on the lock-step schedules.
bool head_dim_trimmed(int d) { return d == 32 || d == 96 || d == 192; }
bool head_dim_native(int d) { return d == 64 || d == 128 || d == 256 || head_dim_trimmed(d); }
// kernel head dim a call runs on: the next built size.  A head dim between the built sizes (a multiple of 8: 40, 72, 80, 104, 160, 224, ..)
// runs with a run-time column bound (FwdK / BwdK::d_chunks: the chunks behind the head dim read as zeros and are never stored; lock-step
// forward, 4-wave dQ kernel, dK/dV kernel, delta pre-pass) -- the reference rounds internally and masks columns the same way
// (flash_api.cpp:458,872, Is_even_K); no padded copies anywhere.
int head_dim_kernel(int d) { for (int n : {32, 64, 96, 128, 192}) if (d <= n) return n; return 256; }
int head_dim_pitch(int d) { return d <= 64 ? 64 : d <= 128 ? 128 : 256; }  // row pitch of tiles and of split-KV partial rows

// Reference flash_api.cpp:422-427 (+ :155-162): windows at least as wide as the key sequence are
// unbounded, a single query row needs no causal mask, causal means window_right = 0.
void normalize_window(int seqlen_q, int seqlen_k, bool has_alibi, int& is_causal, int& wl, int& wr) {
  if (wl >= seqlen_k) wl = -1;
  if (wr >= seqlen_k) wr = -1;
  if (seqlen_q == 1 && !has_alibi) is_causal = 0;
  if (is_causal) wr = 0;
  if (wl < 0) wl = -1;
  if (wr < 0) wr = -1;
}

// Split-KV schedule of the decode path (reference num_splits_heuristic, flash_api.cpp:275-347, re-derived for 256 CUs
// with two workgroups each): split only single-block query lengths whose (batch x head) grid leaves most CUs idle,
// into the fewest key splits that give every CU two workgroups; a split is a whole number of 64-key tiles.
// Head packing on the fixed-length forward and the KV-cache path (FwdK::pack_g; the reference packs only the single-row decode step by reshaping q,
// flash_api.cpp:429-437 -- FA3 generalises it as PackGQA, hopper/pack_gqa.h): when all g query heads of a KV group times the
// query rows fit one 128-row block, the group's heads become rows of that block and K/V are streamed once per KV head instead
// of once per query head.  Returns g (1 = no packing).
// The absorbed MLA decode pair (fa_fwd_mla.hip): q / k head dim 576, v / o head dim 512.  Its kernel ALWAYS runs the packed-row layout, in as many 64-row
// blocks as g * seqlen_q needs (unpacked, 128 heads would stream the cache 128 times).
inline bool mla_pair(int d, int d_v) { return d == 576 && d_v == 512; }
constexpr int kMlaBlockRows = 64;
int pack_group(const FaFwdParams* a) {
  const int g = a->h_k > 0 ? a->h / a->h_k : 1;
  if (mla_pair(a->d, a->d_v)) return g > 1 ? g : 1;
  if (g <= 1 || !fa::knobs().pack_gqa || (a->d_v > 0 && a->d_v != a->d) || a->cu_seqlens_q || a->seqused_q || a->p_dropout > 0.f || a->seqlen_q < 1 || (long)a->seqlen_q * g > 128) return 1;
  return g;
}
int choose_splits(const FaFwdParams* a, int& split_tiles) {
  const int tiles = (a->seqlen_k + 63) / 64;
  split_tiles = tiles;
  if (mla_pair(a->d, a->d_v)) {
    // keys are split while the packed rows of a KV head fit the 128 rows every other kernel's rule allows (one or two 64-row blocks); one workgroup per CU:
    // the fewest splits that give each of the 256 CUs a workgroup, at least 4 tiles per split.  (A choice by arithmetic, not a measurement.)
    const long rows = (long)a->seqlen_q * pack_group(a);
    if (rows > 128 || rows < 1 || tiles < 2 || a->num_splits == 1) return 1;
    int want = a->num_splits;
    if (want <= 0) {
      const long units = (long)a->b * a->h_k * ((rows + kMlaBlockRows - 1) / kMlaBlockRows);
      if (units >= 192) return 1;
      want = (int)((256 + units - 1) / units);
      want = std::min(want, std::max(1, tiles / 4));
    }
    want = std::max(1, std::min(std::min(want, 64), tiles));   // (64: fa_splitkv_combine_kernel reads one split per lane -- B = 1, H = 128 gets 2 x 64 = 128 workgroups, half the CUs)
    split_tiles = (tiles + want - 1) / want;
    return (tiles + split_tiles - 1) / split_tiles;
  }
  if (a->seqlen_q > 128 || tiles < 2 || a->num_splits == 1) return 1;
  int want = a->num_splits;
  if (want <= 0) {
    const long units = (long)a->b * a->h / pack_group(a);   // workgroups of the unsplit grid
    if (units >= 384) return 1;
    want = (int)((512 + units - 1) / units);
    want = std::min(want, std::max(1, tiles / 4));  // at least 4 tiles (256 keys) per split
  }
  want = std::max(1, std::min(std::min(want, 64), tiles));
  split_tiles = (tiles + want - 1) / want;
  return (tiles + split_tiles - 1) / split_tiles;
}
int64_t splitkv_bytes(const FaFwdParams* a, int n_splits) {
  if (n_splits <= 1) return 0;
  const int pitch = mla_pair(a->d, a->d_v) ? 512 : head_dim_pitch(a->d);   // partial rows have the VALUE width
  return (int64_t)n_splits * a->b * a->h * a->seqlen_q * (pitch + 1) * (int64_t)sizeof(float);
}

// Forward schedule code: 64 = 64-rows-per-wave kernel (fa_fwd_w64.hip, 4 waves, 256-row blocks), 34 / 38 = software-pipelined
// kernel (fa_fwd_il.hip) with 4 / 8 waves per workgroup, 4 / 8 = lock-step kernel with 4 / 8 waves, 16 = 8-wave ping-pong
// (fa_fwd.hip).  wl / wr = normalised window.
// The 64-rows-per-wave forward addresses K and V through buffer descriptors with 32-bit byte offsets from the (batch, kv-head)
// base (fa_fwd_w64.hip: launch_fwd_w64): the whole key range of a sequence plus two tiles of overshoot must span < 4 GiB.
// Q and O are addressed the same way over the 256 rows of a query block (q_srd_of / dma_q_piece, the epilogue's lane_off / soff).
bool w64_span_ok(const FaFwdParams* a) {
  const uint64_t rs = (uint64_t)std::max<int64_t>(a->k_row_stride, a->v_row_stride);
  const uint64_t qo = (uint64_t)std::max<int64_t>(a->q_row_stride, a->o_row_stride);
  const uint64_t keys = a->block_table ? 64 : (a->seqlen_k > 0 ? a->seqlen_k : 1);   // (a paged cache is addressed tile by tile)
  // (paged: the kernel forms a page's and a tile's byte sizes in 32 bits -- fa_fwd_w64.hip pg_bytes_* / tl_bytes_*)
  if (a->block_table) {
    const uint64_t pg = (uint64_t)std::max<int64_t>(a->k_batch_stride, a->v_batch_stride) * 2u;
    if (pg >= (1ull << 32) || (uint64_t)std::max(a->page_block_size, 1) * rs * 2u >= (1ull << 32)) return false;
  }
  return (keys + 128) * rs * 2u < (1ull << 32) && 256ull * qo * 2u < (1ull << 32);
}
int fwd_schedule_nw(const FaFwdParams* a, int wl, int wr) {
  // Schedule (measured on MI355X, tools/ab_bench.py, profiles/r03_fwd_schedules.txt; FA_FWD_NW overrides):
  //   head dim 128, >= 512 query rows: the 64-rows-per-wave kernel (persistent 256-row workgroups, one per CU) from 8 key tiles of 64
  //   keys per query block on average, as long as its 256-row blocks still fill the chip (>= 200 of them; key loops of >= 32 tiles
  //   -- non-causal S >= 2048, causal S >= 4096, config 3 included -- take it regardless).  With round 3's per-block costs (one
  //   iteration body, 7k-clock prologue) it beats the 4-wave pipelined kernel by 7 % at S = 1024, 14-21 % at S = 2048 and 19-23 %
  //   from S = 4096 (1.20-1.24 vs 1.01-1.03 PFLOP/s non-causal); at S = 512 the two tied until round 5 peeled a wave's first and last
  //   iteration (fixed-length batches under a right bound now take it from 4 visible tiles on average, see below).  Shorter loops and small grids stay on the
  //   4-wave pipelined kernel (Q fragments in registers, two 128-row workgroups per CU hide each other's prologue / epilogue).
  //   FA_STRICT keeps the pipelined kernels (fp32 scaling of every score).  D = 64 has half the MFMA work per softmax element: the
  //   64-rows-per-wave kernel wins from 32 key tiles on average without a right bound (S >= 2048: +1 %, S >= 4096: +12-16 %) and from
  //   16 under a causal mask (S = 2048: +12 %, S = 1024: -3 %).
  //   K/V views whose key range spans >= 4 GiB (w64_span_ok) fall back from the 64-rows-per-wave kernel to the pipelined one,
  //   which addresses tile by tile.
  int nw = fa::knobs().fwd_nw;
  if (nw != 4 && nw != 8 && nw != 16 && nw != 34 && nw != 38 && nw != 64) {
    const bool right_bounded = (wr >= 0);
    const long avg_keys = right_bounded ? (a->seqlen_k + 1) / 2 : a->seqlen_k;
    const long span = (wl >= 0) ? std::min<long>(avg_keys, wl + (wr >= 0 ? wr : a->seqlen_k) + 256) : avg_keys;
    const long tiles = span / 64;
    const long blocks256 = a->cu_seqlens_q ? (long)a->h * (a->total_q / 256 + 1) : (long)a->b * a->h * ((a->seqlen_q + 255) / 256);
    const bool fills = blocks256 >= 200;
    const int fallback = a->seqlen_q > 128 ? 34 : 4;
    if (a->d == 128) {
      const bool long_loop = tiles >= 32 && a->seqlen_q >= 512;
      if (fa::knobs().strict) nw = long_loop ? (tiles >= 48 ? 38 : 34) : fallback;
      // (a left window bound keeps the old threshold: both ends of its short key range are masked iterations, and the early waves of a
      // block idle at both -- config 5, 20 tiles per block: 792 TFLOP/s on the pipelined kernel against 741-763 on this one)
      // (round 5: under a right bound from 4 tiles on average -- causal S = 512 -- since a wave's first and last iteration are peeled: 431 against 383 TFLOP/s there,
      // profiles/r05_fwd_w64_peel.txt; without a right bound 4-7 tiles means 256-448 keys in all, and a packed batch is sized here by its LONGEST sequence (its
      // short ones would leave most of a 256-row block empty): neither was measured, the old threshold stands for both)
      else nw = (long_loop || (tiles >= ((right_bounded && !a->cu_seqlens_q) ? 4 : 8) && wl < 0 && a->seqlen_q >= 512 && fills)) ? 64 : fallback;
    } else if (a->d == 64) {
      const long need = right_bounded ? 16 : 32;
      nw = (!fa::knobs().strict && a->seqlen_q >= 512 && (tiles >= 64 || (tiles >= need && fills))) ? 64 : fallback;
    } else {
      nw = fallback;
    }
    if (nw == 64 && !w64_span_ok(a)) nw = 38;   // (only the heuristic falls back: a forced FA_FWD_NW=64 reaches the launcher's -3 and its message)
  }
  return nw;
}

// varlen work list: worth a pre-pass when a max_seqlen-sized grid would be mostly empty slots
// (min_dense: the smallest dense grid, in blocks per head, for which the pre-pass is launched.  64 is the measured choice of the kernels that launch the dense grid
// whatever the list says.  The kernel for a v head dim of its own sizes its grid from the list (work_bound * h workgroups, as fa_fwd_il does), so the list saves it
// launches at any size; its 32 is a choice, not a measurement)
int64_t varlen_list_entries(const FaFwdParams* a, int bm, int min_dense = 64) {
  if (fa::knobs().varlen_list == 0) return 0;  // debugging switch: always the dense grid
  const int64_t dense = (int64_t)a->b * ((a->seqlen_q + bm - 1) / bm);
  const int64_t bound = (int64_t)a->total_q / bm + a->b;
  return (dense * 4 > bound * 5 && dense >= min_dense) ? bound : 0;
}
constexpr int kDvListMinDense = 32;

inline int value_dim(int d, int d_v) { return d_v > 0 ? d_v : d; }

inline bool own_value_dim(int d, int d_v) { return d_v > 0 && d_v != d; }

// What the heuristic's pick becomes once the features have had their say (plan_fwd, for every 16-bit entry point and fa_fwd_schedule_query):
//   64 = the 64-rows-per-wave kernel: plain attention, ALiBi under a right bound on the diagonal (its FEAT_ALIBI variant: the bias rides in the
//        score chains' C operand, key tiles walked downwards), or softcap (FEAT_CAP, round 5: seven vector instructions per score, staged over three
//        gaps), dropout without the random-byte output (FEAT_DROP, round 5: eight Philox calls per step spread two rounds per gap), and plain attention over
//        a paged cache (round 5: a buffer descriptor per 64-key tile); anything else that asked for it runs the 8-wave lock-step kernel on the same 256-row blocks;
//   34 / 38 = the software-pipelined kernel with 4 / 8 waves: plain attention only, else the lock-step kernel with the same wave count.
int resolve_fwd_features(const FaFwdParams* a, int nw, int wr, int n_splits, int pack, bool bounded, bool& w64, bool& il) {
  const bool shape_ok = n_splits == 1 && pack == 1 && !bounded;
  const bool base0 = !(a->p_dropout > 0.f) && shape_ok;
  const bool base = base0 && !(a->softcap > 0.f);
  const bool plain = base && !a->alibi_slopes;
  const bool w64_alibi = base && a->alibi_slopes && wr == 0;
  const bool w64_cap = base0 && a->softcap > 0.f && !a->alibi_slopes;
  const bool w64_drop = shape_ok && a->p_dropout > 0.f && !a->randval && !(a->softcap > 0.f) && !a->alibi_slopes && !a->block_table;   // (no random-byte output there)
  // (a paged cache: the plain variant only, and not together with a batch index or left padding -- the API rejects those combinations anyway)
  const bool paged_ok = !a->block_table || (plain && !a->cache_batch_idx && !a->leftpad_k && a->page_block_size % 64 == 0);
  w64 = nw == 64 && (plain || w64_alibi || w64_cap || w64_drop) && paged_ok;
  if (nw == 64 && !w64) nw = 8;
  il = (nw == 34 || nw == 38) && plain;
  if ((nw == 34 || nw == 38) && !il) nw -= 30;
  return nw;
}

// ---- the forward plan ----
enum FwdEntry { kFaFwd, kFaVarlenFwd, kFaFwdKvcache, kFaFwdFp8, kFaVarlenFwdFp8, kFaFwdKvcacheFp8 };
enum FwdFamily { kFamLockstep, kFamPipelined, kFamW64, kFamDv, kFamMla, kFamFp8, kFamFp8Kv };
struct FwdPlan {
  FwdFamily family;
  int schedule;                   // the code fa_fwd_schedule_query returns (see fwd_schedule_nw); for the lock-step and pipelined families also the launcher's wave count (+ 30)
  int dk; bool bounded;           // kernel head dim; a run-time column bound (FwdK::d_chunks)
  int bm;                         // query rows per workgroup
  int pack;                       // pack_group: query heads of a KV group in the rows of a block (1 = none)
  int wl, wr;                     // normalised window
  int want_splits, n_splits, split_tiles, split_pitch;   // key splits the schedule asks for / the workspace grants (1 = unsplit), key tiles per split, pitch of a partial row
  int64_t split_bytes;            // ... and their workspace; a forced num_splits > 1 without it is refused (want_splits > 1, n_splits == 1, FaFwdParams::num_splits > 1)
  int64_t list_entries; bool list;   // work-list entries of an uneven packed batch (0 = the dense grid) and whether the workspace holds them
  int64_t ws_bytes;               // the workspace the call can use
};
constexpr int64_t kAnyWorkspace = INT64_MAX;   // on offer to a query: as much as the plan asks for

// `offered`: bytes of caller workspace (0 without one); `sizing`: the caller reads ws_bytes alone.  The plan depends on it: without room for the partial rows an automatic split runs unsplit (and the 16-bit
// KV-cache path keeps its schedule: nw = 4 is forced only by a granted split), without room for the work list the dense grid runs.
FwdPlan plan_fwd(const FaFwdParams* a, FwdEntry e, int64_t offered, bool sizing = false) {
  FwdPlan p{};
  const bool fp8 = e >= kFaFwdFp8, varlen = e == kFaVarlenFwd || e == kFaVarlenFwdFp8, kvcache = e == kFaFwdKvcache || e == kFaFwdKvcacheFp8;
  const bool mla = kvcache && mla_pair(a->d, a->d_v), own_dv = own_value_dim(a->d, a->d_v);
  int causal = a->is_causal;
  p.wl = a->window_left; p.wr = a->window_right;
  normalize_window(a->seqlen_q, a->seqlen_k, a->alibi_slopes != nullptr, causal, p.wl, p.wr);
  // (fa_fwd too: a short query chunk with grouped heads is the same problem without a cache -- FA3's PackGQA covers prefill, hopper/pack_gqa.h;
  // packed varlen batches keep one block per head; the fixed-length fp8 kernel has no packed-row layout)
  p.pack = (varlen || e == kFaFwdFp8) ? 1 : pack_group(a);
  p.dk = head_dim_kernel(a->d);   // kernel head dim; != a->d: run-time column bound
  p.bounded = p.dk != a->d;
  p.n_splits = p.want_splits = 1;
  // decode: split the keys over several workgroups when (batch x heads) cannot fill the chip
  if (kvcache) {
    p.want_splits = choose_splits(a, p.split_tiles);
    p.split_pitch = mla_pair(a->d, a->d_v) ? 512 : head_dim_pitch(a->d);
    p.ws_bytes = p.split_bytes = splitkv_bytes(a, p.want_splits);
    if (p.want_splits > 1 && offered >= p.split_bytes) p.n_splits = p.want_splits;   // (else an automatic schedule runs unsplit)
  }
  if (sizing && !varlen) return p;   // (fa_fwd_workspace_bytes on a fixed-length call: ws_bytes is settled, the rest of the plan is not read)
  int min_dense = 64;
  if (fp8) {  // fa_fwd_fp8.hip / fa_fwd_fp8_kv.hip: 4 waves, 128-row blocks
    p.family = kvcache ? kFamFp8Kv : kFamFp8; p.schedule = 4; p.bm = 128;
  } else if (mla) {  // q / k 576, v / o 512 = the latent part of k: fa_fwd_mla_kernel, always packed rows, 64-row blocks, split keys
    p.family = kFamMla; p.schedule = 4; p.bm = kMlaBlockRows;
  } else if (own_dv) {  // q / k 192, v / o 128: fa_fwd_dv_kernel, 4 waves x 32 rows (no key splits, no packing: a launching call is refused before it plans / pack_group)
    p.family = kFamDv; p.schedule = 4; p.bm = 128; min_dense = kDvListMinDense;
  } else {
    int nw = fwd_schedule_nw(a, p.wl, p.wr);
    if (p.pack > 1) nw = 4;  // grouped query heads become rows of one block (4-wave lock-step kernel)
    if (p.dk > 128 || head_dim_trimmed(p.dk) || p.bounded) nw = 4;  // head dim 256: one 4-wave lock-step workgroup per CU (512-register budget); trimmed / bounded dims: 4-wave lock-step
    if (p.n_splits > 1) nw = 4;
    bool w64 = false, il = false;
    p.schedule = resolve_fwd_features(a, nw, p.wr, p.n_splits, p.pack, p.bounded, w64, il);
    p.family = w64 ? kFamW64 : il ? kFamPipelined : kFamLockstep;
    p.bm = w64 ? 256 : il ? 32 * (p.schedule - 30) : fa::fwd_block_m(p.schedule);
  }
  if (varlen) {  // uneven packed batch: enumerate the non-empty query blocks, heaviest first
    p.list_entries = varlen_list_entries(a, p.bm, min_dense);
    p.ws_bytes = p.list_entries > 0 ? (p.list_entries + 1) * 8 : 0;
    p.list = p.list_entries > 0 && offered >= p.ws_bytes;
  }
  return p;
}

// dQ schedule (fa_launch.h Knobs::bwd_dq_nw).  Measured on MI355X (profiles/r02_bwd_schedules.txt): the 64-rows-per-wave
// kernel wins from ~2k keys at head dim 128 (config 3: dQ 955 vs 997 us, S = 16k non-causal 1383 vs 1584 us) and loses on
// short sequences, where its 256-row blocks leave CUs idle.
// What the 64-per-wave backward kernels cover besides plain attention: ALiBi under a causal right bound (the bias is linear in the key there) in both of them;
// softcap in both at head dim 128, dropout in the dQ kernel at head dim 128 -- one feature at a time (round 5; profiles/r05_bwd_features_w64.txt)
bool bwd_w64_features_ok(const FaBwdParams* a, bool dq_kernel) {
  const int n = (a->softcap > 0.f) + (a->p_dropout > 0.f) + (a->alibi_slopes != nullptr);
  if (n > 1) return false;
  if (a->softcap > 0.f) return a->d == 128;                   // (head dim 64: the 4-wave feature kernel measured 2-4 % ahead)
  if (a->p_dropout > 0.f) return dq_kernel && a->d == 128;
  return !a->alibi_slopes || a->is_causal || a->window_right == 0;
}

int bwd_dq_schedule(const FaBwdParams* a) {
  // trimmed head dims (32 / 96 / 192), head dims between the built sizes and head dim 256 only have the 4-wave, 128-row dQ kernel
  // (fa_bwd.hip: launch_dq_f): the block size fill_bwd / bwd_list_entries derive from the schedule has to be that kernel's, whatever the knob says
  if (head_dim_trimmed(head_dim_kernel(a->d)) || !head_dim_native(a->d) || a->d > 128) return 4;
  const int knob = fa::knobs().bwd_dq_nw;
  if (knob == 4 || knob == 8 || knob == 64) return knob;
  const bool plain = bwd_w64_features_ok(a, true);
  if (a->d == 64) {
    // round 4 (profiles/r04_bwd_schedules.txt): at head dim 64 the 64-rows-per-wave kernel wins from ~2k visible keys per query row ON AVERAGE -- non-causal
    // S >= 2048 (+5.5 .. +7.5 % on the whole backward), causal S >= 8192 (+5.6 .. +7.4 %); it ties at causal S = 4096 and loses below
    // mean visible keys per query row: bottom-right aligned, row i sees keys up to i + (sk - sq) + window_right
    const bool right_bounded = a->is_causal || a->window_right >= 0;
    const long wr = a->is_causal ? 0 : a->window_right;
    long avg_keys = a->seqlen_k;
    if (right_bounded) { avg_keys = (long)a->seqlen_k - a->seqlen_q / 2 + wr; if (avg_keys > a->seqlen_k) avg_keys = a->seqlen_k; if (avg_keys < 0) avg_keys = 0; }
    // (late round 6: without a right bound from 1536 keys -- whole backward S = 1536 567 | 583, S = 1792 578 | 596 TFLOP/s, a tie at S = 1024)
    return (plain && a->window_left < 0 && a->seqlen_q >= 512 && avg_keys >= (right_bounded ? 2048 : 1536)) ? 64 : 4;
  }
  if (a->d != 128 || !plain || a->seqlen_q < 512) return 4;
  if (a->seqlen_k >= 2048) return 64;
  // (late round 6: WITHOUT a right bound the 64-rows-per-wave kernel already leads from 768 keys once its 256-row blocks fill the chip -- whole backward, TFLOP/s, 32 rows
  // per wave | 64: S = 768 569 | 591, S = 1024 631 | 650, S = 1280 667 | 702, S = 1536 677 | 720 (B16 H32: 699 | 751), S = 1600 on 448 blocks 569 | 619, GQA 32/8 S = 1024 on
  // 256 blocks 328 | 345; S = 512 500 | 485.  Under a causal mask a tie at S = 1600 (516 | 522) and behind on small grids (S = 1536 on 96 blocks 174 | 165): profiles/r06_bwd_c5.txt (9))
  const bool right_bounded = a->is_causal || a->window_right >= 0;
  const long blocks256 = a->cu_seqlens_q ? 0 : (long)a->b * a->h * ((a->seqlen_q + 255) / 256);
  const bool featureless = a->softcap == 0.f && a->p_dropout == 0.f && !a->alibi_slopes;   // (the feature variants were not measured below 2k keys)
  return (featureless && !right_bounded && a->window_left < 0 && a->seqlen_k >= 768 && blocks256 >= 256) ? 64 : 4;
}

// dK/dV schedule (fa_launch.h Knobs::bwd_dkdv): 64 = four waves x 64 keys (fa_bwd_dkdv_w64.hip; plain attention or causal ALiBi at head dim 64 / 128, softcap at head dim 128), 8 = eight waves x 32 keys
// (fa_bwd.hip: every feature variant, head dim 256, trimmed head dims).  Measured (profiles/r05_bwd_dkdv_w64.txt): at head dim 128 the 64-keys-per-wave kernel
// wins from 2k query rows per key block (+1 % at S = 2048, +3 .. +6 % on the whole backward from S = 4096, GQA included) and loses below (its pipeline fill /
// drain and 160 KB of LDS per workgroup cost more than they save on a short walk); at head dim 64 it ties or loses everywhere.
int bwd_dkdv_schedule(const FaBwdParams* a) {
  const bool plain = bwd_w64_features_ok(a, false);
  if (!plain || !head_dim_native(a->d) || head_dim_trimmed(head_dim_kernel(a->d)) || (a->d != 128 && a->d != 64)) return 8;
  const int knob = fa::knobs().bwd_dkdv;
  if (knob == 8 || knob == 64) return knob;
  if (fa::knobs().dkdv_prescale) return 8;   // (FA_DKDV_PRESCALE=1 names a variant of the eight-wave kernel)
  // (a key block's walk: the query rows that can see it -- bounded by the window under a two-sided mask; packed batches are sized by their longest sequence
  // and stay on the eight-wave kernel below 2k rows of it)
  long walk = a->seqlen_q;
  const int wr = a->is_causal ? 0 : a->window_right;
  const int ratio = a->h / a->h_k;
  if (a->window_left >= 0 && wr >= 0) walk = std::min<long>(walk, (long)a->window_left + wr + 256) * ratio;   // (the query heads of a group are walked one after the other: config 5, 4 x 1280 rows, measured +1.5 % on this kernel)
  // (round 6, late: ... and so they are without a window -- a key block of a GQA group walks ratio x Sq rows, half of them on average under a right bound.  Measured on the
  // pair, TFLOP/s eight-wave | this kernel: causal S = 1024 ratio 4 158-172 | 165-182 (+5 %), ratio 8 168-172 | 178-182 (+6 %), S = 768 ratio 4 +2 %, S = 512 ratio 4 / 8 -2 %;
  // no mask S = 1024 ratio 4 296-306 | 322-332 (+8.5 %), S = 1536 ratio 4 +8 %, S = 640 ratio 8 +10 %: from 2k walked rows on average, not below 640 rows per head)
  else if (a->window_left < 0 && ratio > 1 && a->seqlen_q >= 640 && !a->cu_seqlens_q) walk = std::max<long>(walk, (long)a->seqlen_q * ratio / (wr >= 0 ? 2 : 1));
  // (late round 6: without any mask from 1536 walked rows -- S = 1536 688 | 720, S = 1792 667 | 695 TFLOP/s on the whole backward, S = 1280 / 1024 +1 ... +2 %; under a causal mask a tie below 2k)
  return (a->d == 128 && walk >= ((wr < 0 && a->window_left < 0) ? 1536 : 2048)) ? 64 : 8;
}

// varlen backward work lists: query blocks for the dQ kernel, key blocks for the dK/dV kernel (entries each, 0 = dense grids)
void bwd_list_entries(const FaBwdParams* a, int bm, int bn, int64_t& q_entries, int64_t& k_entries) {
  q_entries = k_entries = 0;
  if (!a->cu_seqlens_q || !a->cu_seqlens_k || fa::knobs().varlen_list == 0) return;
  const int64_t dq_dense = (int64_t)a->b * ((a->seqlen_q + bm - 1) / bm), dq_bound = (int64_t)a->total_q / bm + a->b;
  const int64_t dk_dense = (int64_t)a->b * ((a->seqlen_k + bn - 1) / bn), dk_bound = (int64_t)a->total_k / bn + a->b;
  if (dq_dense * 4 > dq_bound * 5 && dq_dense >= 64) q_entries = dq_bound;
  if (dk_dense * 4 > dk_bound * 5 && dk_dense >= 64) k_entries = dk_bound;
}

// (Round 2's two-launch dS-spill backward, FA_BWD_MODE=2 -- a tie with the recomputing pair, profiles/r02_bwd_5_vs_7_contractions.txt, on O(S^2) scratch -- is
// superseded by FA_BWD_MODE=5 below: the same idea on the 64-per-wave kernels with a bounded workspace; git history keeps the old experiment.)
// Fused backward (FA_BWD_MODE=3, fa_bwd.hip fa_bwd_fused_kernel): bytes of the dS workspace (256-B aligned) when the call qualifies, else 0; the sync
// area (fa_kernel_params.h FZ_*) sits behind it.  Same conditions as launch_bwd_fused.
// Round 6: it is the DEFAULT (FA_BWD_MODE=0) where it was measured ahead of the recomputing pair and its workspace stays within bounds (bwd_fused_plan below; profiles/r06_bwd_c5.txt (5), timed
// WITHOUT the status read -- a stream sync per call, which the default path does not do and which cost the launch 9 % at S = 1024): head dim 128, Sq = Sk, at least
// 32 (batch, kv head) units, under a causal mask from 512 to 4096 rows (+8 % / +18 % / +15 % at S = 512 / 1024 / 2048 on the sweep's shapes, +7 ... +9 % at S = 3072 and
// +9 ... +13 % at S = 4096 on the grids that fit the 1 GiB -- 32 heads) and -- until the pair's dQ half got the 64-rows-per-wave kernel below 2k keys, see the return below -- without a mask from 512 to 1536 rows (+1.5 % / +5 % / +5.6 % / +3 ... +5 % at 512 / 768 / 1024 / 1536).
// Where the workspace would exceed 1 GiB it ties or loses anyway (config 3: a tie on 4 GiB; S = 4096 on 64 heads +3 % on 2 GiB; S = 8192 -8 %); without a mask from
// S = 2048 -6 ... -10 %; head dim 64 without a mask -20 % (causal +3 % / -1 %: left to the pair); small grids (16 units) -3 %.
// FA_BWD_MODE=3 forces it wherever it applies (cap FA_BWD_DS_CAP_MB), -1 / 1 never.
bool bwd_fused_by_table(const FaBwdParams* a) {
  int causal = a->is_causal, wl = a->window_left, wr = a->window_right;
  normalize_window(a->seqlen_q, a->seqlen_k, false, causal, wl, wr);
  if (a->d != 128 || wl >= 0 || a->seqlen_q != a->seqlen_k || (long)a->b * a->h_k < 32) return false;
  if (fa::knobs().bwd_dq_nw != 0 || fa::knobs().bwd_dkdv != 0 || fa::knobs().dkdv_prescale || fa::knobs().strict) return false;
  const int s = a->seqlen_q;
  // (late round 6, sync-free timings at large batches: from 256 to 511 rows the launch leads once the grid is large -- causal S = 256: 512 units a tie, 1024 +4 %, 1536 +7 %,
  // 2048 +10 %; S = 320 / 384 on 1024 units +15 % / +13 %, S = 384 / 448 on 512 units +7 % / +9 %, S = 384 on 256 units a tie; S = 128 -5 %; no mask S = 256 / 384 on 2048 units
  // +3 % / +7 %, S = 384 on 512 units +1 %: profiles/r06_bwd_c5.txt (8))
  if (s >= 256 && s < 512) { const long us = (long)a->b * a->h_k * s; return wr == 0 ? us >= 196608 : (wr < 0 && us >= 786432); }
  // (without a mask from 512 rows: the pair, whose dQ half takes the 64-rows-per-wave kernel from 768 keys since late round 6 -- bwd_dq_schedule -- and is then level with
  // this launch or ahead of it at no workspace: S = 768 569 fused | 591 pair, 1024 658 | 650, 1280 696 | 702, 1536 698 | 720, B16 H32 S = 1536 739 | 751; S = 512 a tie on either dQ kernel)
  return wr == 0 && s >= 512 && s <= 4096;
}
// The row packing of a dS workspace, of the fused launch and of the chunked 5-contraction backward alike: rows of 64-key pairs (fa_device.h ds_row_start):
// c1 - 1 = key sub-tiles row block 0 sees (keys <= 31 + (sk - sq) + wr), jb = the first row block that holds every pair, head_tiles = sub-tiles of 2 KB per head.
struct DsPack { int np64, c1, jb, head_tiles; };
DsPack ds_pack(int sq, int sk, int wr) {
  DsPack f;
  f.np64 = (sk + 63) / 64;
  f.c1 = wr >= 0 ? (int)std::min<int64_t>(2 * f.np64, ((int64_t)31 + (sk - sq) + wr) / 32 + 2) : 2 * f.np64;
  f.jb = std::max(0, 2 * f.np64 - f.c1);
  f.head_tiles = fa::ds_row_start((sq + 31) / 32, f.c1, f.jb, f.np64);
  return f;
}
// The fused launch's plan (round 6, late): the batch is cut into chunks of whole batch entries so that a chunk's packed dS fits the cap, one launch per chunk on the
// SAME workspace (stream order: launch c + 1 starts when launch c is over).  By the table (mode 0) the cap is 1.25 GiB (the packed triangle of the shapes whose half
// square is exactly 1 GiB comes to 1.03 - 1.08 GiB: B8 S2048 H32 +15 %, B4 S4096 H16 +3 %, B4 S3072 H32 +7 %), a chunk keeps >= 32 (batch, kv head) units, and only
// sequences up to 2048 rows are chunked -- there the launch is 12 ... 25 % ahead of the pair at any grid size (B32 S1024 H32: 524 against 418 TFLOP/s, B16 S2048 H32
// 652 / 583, B64 S512 H32 366 / 313, no mask B32 S1024 H32 698 / 649; profiles/r06_bwd_c5.txt (7)); from 2048 to 4096 rows it is only ahead of the pair ON THE
// SAME GRID (+3 ... +9 %) and the pair gains more from a larger grid than that, so there the whole batch has to fit.  FA_BWD_MODE=3: cap FA_BWD_DS_CAP_MB, chunked whenever needed.
struct FusedPlan { int nb, n_chunks; int64_t ds_bytes, sync_bytes; DsPack pack; };   // batch entries per chunk, chunks, bytes of a chunk's dS / sync area, row packing
bool bwd_fused_plan(const FaBwdParams* a, FusedPlan& pl) {
  pl = FusedPlan{};
  const int mode = fa::knobs().bwd_mode;
  if ((mode != 3 && mode != 0) || a->cu_seqlens_q || a->cu_seqlens_k || a->seqused_q || a->seqused_k || (a->d != 128 && a->d != 64)) return false;
  if (a->seqlen_q <= 0 || a->seqlen_k < a->seqlen_q || a->window_left >= 0 || a->softcap > 0.f || a->alibi_slopes || a->p_dropout > 0.f || a->b <= 0) return false;
  if (mode == 0 && !bwd_fused_by_table(a)) return false;
  // (packed rows, fa_device.h ds_row_start -- a causal mask stores its triangle: about half of B*H*Sq*Sk*2 bytes)
  int causal = a->is_causal, wl = a->window_left, wr = a->window_right;
  normalize_window(a->seqlen_q, a->seqlen_k, false, causal, wl, wr);
  const DsPack fp = pl.pack = ds_pack(a->seqlen_q, a->seqlen_k, wr);
  const int64_t per_batch = (int64_t)a->h * fp.head_tiles * 2048;
  const int64_t cap = mode == 0 ? ((int64_t)1280 << 20) : ((int64_t)fa::knobs().bwd_ds_cap_mb << 20);
  int64_t nb = std::min<int64_t>(a->b, cap / per_batch);
  if (nb < 1) return false;
  const int n_chunks = (int)((a->b + nb - 1) / nb);
  nb = (a->b + n_chunks - 1) / n_chunks;   // (even chunks)
  if (mode == 0 && n_chunks > 1 && (a->seqlen_q > 2048 || (a->b - (n_chunks - 1) * nb) * a->h_k < 32)) return false;   // (the last chunk is the smallest)
  pl.nb = (int)nb; pl.n_chunks = n_chunks;
  pl.ds_bytes = (nb * per_batch + 255) & ~(int64_t)255;
  pl.sync_bytes = fa::fz_sync_words(nb * a->h * ((a->seqlen_q + 255) / 256), fa::knobs().fz_line) * 4;
  return true;
}

// ---- 5-contraction backward (round 6; reference: ONE pass forms S, dP and dS and all three gradients follow from it, csrc/flash_attn/src/flash_bwd_kernel.h:457-733) ----
// The 64-keys-per-wave dK/dV items write dS (input dtype) to a workspace, dQ = dS.K is one contraction instead of the recomputing dQ kernel's three.  The workspace is
// bounded: the (batch, kv head) units are cut into chunks of whole XCD rounds (8 units), launch c runs the dK/dV items of chunk c and the dQ items of chunk c - 1
// in one grid (stream order is the hand-off, nothing spins), two slots alternate.  Rows of a slot are packed (fa_device.h ds_row_start): a causal mask stores its triangle only.
struct C5Plan {
  int hpx, rounds, rounds_per_chunk, n_chunks;
  int nq32, nk32, nmb, nnb;
  DsPack pack;
  int64_t slot_bytes;
};
bool bwd_c5_plan(const FaBwdParams* a, C5Plan& pl) {
  const int mode = fa::knobs().bwd_mode;
  if (mode != 0 && mode != 5) return false;
  if (a->cu_seqlens_q || a->cu_seqlens_k || a->seqused_q || a->seqused_k || (a->d != 128 && a->d != 64)) return false;
  if (a->softcap > 0.f || a->alibi_slopes || a->p_dropout > 0.f || a->seqlen_q <= 0 || a->seqlen_k < a->seqlen_q || a->b <= 0) return false;
  if (fa::knobs().bwd_dkdv == 8 || fa::knobs().dkdv_prescale) return false;   // (knobs that name the eight-wave dK/dV kernel)
  int causal = a->is_causal, wl = a->window_left, wr = a->window_right;
  normalize_window(a->seqlen_q, a->seqlen_k, false, causal, wl, wr);
  if (wl >= 0) return false;
  pl.nq32 = (a->seqlen_q + 31) / 32; pl.nk32 = (a->seqlen_k + 31) / 32;
  pl.nmb = (a->seqlen_q + 255) / 256; pl.nnb = (a->seqlen_k + 255) / 256;
  pl.pack = ds_pack(a->seqlen_q, a->seqlen_k, wr);
  const int n_units = a->b * a->h_k, ratio = a->h / a->h_k;
  pl.hpx = (a->h_k % 8 == 0) ? a->h_k / 8 : 0;
  pl.rounds = (n_units + 7) / 8;
  const int64_t round_bytes = (int64_t)8 * ratio * pl.pack.head_tiles * 2048;
  const int64_t slot_cap = ((int64_t)fa::knobs().bwd_c5_cap_mb << 20) / 2;
  if (round_bytes > slot_cap || round_bytes >= ((int64_t)1 << 32)) return false;
  int rpc = (int)std::min<int64_t>(pl.rounds, slot_cap / round_bytes);
  while ((int64_t)rpc * round_bytes >= ((int64_t)1 << 32)) --rpc;   // (32-bit buffer offsets inside a slot)
  pl.n_chunks = (pl.rounds + rpc - 1) / rpc;
  pl.rounds_per_chunk = (pl.rounds + pl.n_chunks - 1) / pl.n_chunks;   // balanced
  pl.slot_bytes = ((int64_t)pl.rounds_per_chunk * round_bytes + 255) & ~(int64_t)255;
  if (mode == 5) return true;
  return false;   // (the measured table goes here)
}

// GQA group split (late round 6).  The dK/dV kernels own (batch, kv head, key block) items and walk the group's query heads inside: with few kv heads and a small batch
// the grid does not fill the chip (B2 S1024 H32/2: 16 workgroups on 256 CUs, 55 TFLOP/s).  The group is then split into gs = 2^n virtual kv heads -- consecutive query
// heads each, BwdK::kv_in_shift tells the kernels which real K / V head to read --, their partial dK / dV go to a workspace [b][sk][h_k * gs][d] in the input dtype and
// one small kernel sums them (the reference's own form: per-query-head dK / dV summed by at::sum_out, flash_api.cpp:1000-1004).  Fixed-length batches, head dims the
// kernels hold natively; gs = the smallest power of two (<= 8) that brings the grid to 1024 workgroups, or the whole group.
struct GsplitPlan { int gs, shift; int64_t bytes, dk_bytes; };
bool bwd_gsplit_plan(const FaBwdParams* a, GsplitPlan& pl) {
  pl = GsplitPlan{1, 0, 0, 0};
  if (fa::knobs().bwd_gsplit == 0 || a->cu_seqlens_q || a->cu_seqlens_k || a->seqused_q || a->seqused_k || a->h_k <= 0 || a->h % a->h_k != 0 || a->d % 8 != 0 || !head_dim_native(a->d)) return false;
  const int ratio = a->h / a->h_k;
  if (ratio < 2 || a->seqlen_k <= 0 || a->seqlen_q <= 0 || a->b <= 0) return false;
  const long wgs = (long)a->b * a->h_k * ((a->seqlen_k + fa::bwd_block_n(a->d) - 1) / fa::bwd_block_n(a->d));
  int gs = 1, shift = 0;
  // (under a right bound alone the items are uneven -- 1024 of them; with a left window or no mask they are uniform and short walks pay for the split's extra K / V loads
  // and partials: config 5, 512 items, 0.994 -> 1.055 ms with a split in two; B1 S8192 H32/8 window 1024 0.502 -> 0.578 -- so there only a grid under 256 items is split)
  const long target = ((a->is_causal || a->window_right >= 0) && a->window_left < 0) ? 1024 : 256;
  if (fa::knobs().bwd_gsplit > 1) { while (gs * 2 <= fa::knobs().bwd_gsplit && ratio % (gs * 2) == 0) { gs *= 2; ++shift; } }   // (forced, for tests)
  else { while (wgs * gs < target && gs < 8 && ratio % (gs * 2) == 0) { gs *= 2; ++shift; } }   // (measured, profiles/r06_bwd_gsplit.txt: past 8 virtual heads nothing is gained; 512 uneven causal items on 256 CUs still gain 10 % from a split in two)
  if (gs < 2) return false;
  pl.gs = gs; pl.shift = shift;
  // (dK partials of width d, then dV partials of the value width -- = d unless FaBwdParams::d_v says otherwise)
  pl.dk_bytes = ((int64_t)a->b * a->seqlen_k * a->h_k * gs * a->d * 2 + 255) & ~(int64_t)255;
  pl.bytes = pl.dk_bytes + (((int64_t)a->b * a->seqlen_k * a->h_k * gs * value_dim(a->d, a->d_v) * 2 + 255) & ~(int64_t)255);
  return true;
}
// ---- the backward plan ----
// One order: the chunked 5-contraction launches (FA_BWD_MODE=5), else the fused launch (FA_BWD_MODE=3, or 0 by its table), else the recomputing pair.  `kind` is
// the first of them that applies AND whose workspace is on offer; the pair's own fields (schedules, block sizes, group split, work lists) are always filled in:
// it is also what runs when a launcher finds that its path does not apply after all (-2).
struct BwdPlan {
  int kind;                  // 5 / 3 / 0 (the value LastSchedule::bwd_spill and fa_bwd_plan_query's first word report)
  C5Plan c5; FusedPlan fused;
  int dq_nw, dkdv;           // the pair: dQ schedule (bwd_dq_schedule), dK/dV schedule (bwd_dkdv_schedule, of the split group when it is split)
  int bm, bn;                // query rows per dQ workgroup, key rows per dK/dV workgroup
  GsplitPlan gsplit; bool split;   // the GQA group split and whether it runs (it applies and its workspace is on offer)
  int64_t q_entries, k_entries; bool lists;   // varlen work lists (bwd_list_entries) and whether the workspace holds them
  int64_t ws_bytes;          // the workspace the call can use
};
BwdPlan plan_bwd(const FaBwdParams* a, int64_t offered, bool sizing = false) {
  BwdPlan p{};
  const bool c5 = bwd_c5_plan(a, p.c5), fused = !c5 && bwd_fused_plan(a, p.fused);
  const bool gs = bwd_gsplit_plan(a, p.gsplit);
  p.dq_nw = bwd_dq_schedule(a);
  p.bm = a->d > 128 ? 128 : fa::bwd_block_m(p.dq_nw);
  p.bn = fa::bwd_block_n(a->d);
  bwd_list_entries(a, p.bm, p.bn, p.q_entries, p.k_entries);
  const int64_t list_bytes = (p.q_entries ? (p.q_entries + 1) * 8 : 0) + (p.k_entries ? (p.k_entries + 1) * 8 : 0);   // (work lists: varlen only)
  // (a split GQA group's partial dK / dV are optional like the dS area: without them the unsplit kernels run)
  p.ws_bytes = c5 ? 2 * p.c5.slot_bytes : fused ? p.fused.ds_bytes + p.fused.sync_bytes : gs ? p.gsplit.bytes : list_bytes;
  p.kind = (c5 && offered >= p.ws_bytes) ? 5 : (fused && offered >= p.ws_bytes) ? 3 : 0;
  p.split = gs && offered >= p.gsplit.bytes;
  p.lists = list_bytes > 0 && offered >= list_bytes;
  if (sizing) return p;   // (fa_bwd_workspace_bytes: ws_bytes is settled, the dK/dV schedule is not read)
  if (a->h_k <= 0 || own_value_dim(a->d, a->d_v)) {   // (a v head dim of its own: never the 64-keys-per-wave kernel, it is not built for the pair)
    p.dkdv = 8;
  } else if (p.split) {   // (the dK/dV schedule looks at the walk of a VIRTUAL kv head's group)
    FaBwdParams a2 = *a;
    a2.h_k = a->h_k * p.gsplit.gs;
    p.dkdv = bwd_dkdv_schedule(&a2);
  } else {
    p.dkdv = bwd_dkdv_schedule(a);
  }
  return p;
}

}  // namespace
