// Block geometry of the forward kernels that give a wave 32 query rows (fa_fwd_dv.hip, fa_fwd_fp8.hip, fa_fwd_fp8_kv.hip): which
// (batch, head, query block[, key split]) a workgroup is, what its sequence looks like, and which keys a range of its queries can see.
// fa_fwd_kernel (fa_fwd.hip), the user of every feature below, still spells the same lines out -- its register budget is pinned -- and mirrors this file;
// leftpad_k is its alone and is not handled here.
//
// Every kernel's host contract excludes some arguments (fa_api.cpp refuses them before the launch).  The template int F names the ones a
// kernel admits (FB_* below); code for the others is not generated, so no kernel pays for a branch its contract rules out.
#pragma once
#include "fa_device.h"
#include "fa_kernel_params.h"

namespace fa {

enum {
  FB_LIST = 1,      // varlen work list (FwdK::work_list)
  FB_VARLEN = 2,    // cu_q / cu_k
  FB_SEQUSED = 4,   // seqused_q / seqused_k (padded batches)
  FB_CACHE = 8,     // KV cache: seqused_k + seqused_add, kv_batch_idx, block_table
  FB_SPLIT = 16,    // key splits (FwdK::n_splits)
  FB_SCALAR = 32    // the decoded indices go back to scalar registers (their divisions run on the vector unit), so that what they index --
                    // a page table -- is read with scalar loads
};

// ---- which (batch, head, query block, key split) ----------------------------------------------------------------------------------
struct FwdWork {
  int b, h, m_block, split;
};
// The work list names non-empty blocks only, heaviest first (fa_varlen_schedule_kernel); the dense grid goes through xcd_interleave, key
// splits of one query block are adjacent work items, and under a right-bounded mask the heavy (late) query blocks run first.
// Returns false for a padding workgroup of the grid.
template <int F> FA_DEVINL bool fwd_work(const FwdK& p, int bid, FwdWork& k) {
  auto uni = [](int x) __attribute__((always_inline)) { return (F & FB_SCALAR) ? __builtin_amdgcn_readfirstlane(x) : x; };
  k.split = 0;
  if ((F & FB_LIST) && p.work_list) return work_list_item(p.work_list, bid, p.h, p.h_k, k.b, k.h, k.m_block);
  const int w = xcd_interleave(bid, p.n_units, p.unit_size, p.unit_hpx);
  if (w < 0) return false;
  const int nmbs = (F & FB_SPLIT) ? p.nmb * p.n_splits : p.nmb;  // n_splits >= 1
  const int bh = w / nmbs;
  int mbr = w - bh * nmbs;
  if (F & FB_SPLIT) {
    k.split = uni(mbr % p.n_splits);
    mbr /= p.n_splits;
  }
  k.m_block = uni((p.wr >= 0) ? (p.nmb - 1 - mbr) : mbr);
  k.b = uni(bh / p.h);
  k.h = uni(bh) - k.b * p.h;
  return true;
}

// ---- the sequence of batch entry b ------------------------------------------------------------------------------------------------
struct FwdSeq {
  int sq, sk;        // rows of q (packed heads: g * queries) and keys in use
  int64_t q_row0;    // first row of this sequence in the packed q / o / lse (varlen)
  int64_t q_off, k_off, v_off, o_off;  // element offset of the sequence's first row in q / k / v / o, head 0 (paged cache: k_off = v_off = 0)
};
template <int F> FA_DEVINL FwdSeq fwd_seq(const FwdK& p, int b) {
  constexpr bool VARLEN = (F & FB_VARLEN) != 0, CACHE = (F & FB_CACHE) != 0;
  FwdSeq s;
  s.sq = p.sq;
  s.sk = p.sk;
  s.q_row0 = 0;
  int64_t k_row0 = 0;
  const int bkv = (CACHE && p.kv_batch_idx) ? p.kv_batch_idx[b] : b;  // KV-cache row of this batch entry
  const bool paged = CACHE && p.block_table;                          // the page index supplies the first-dimension offset and the rows
  int64_t q_boff = (int64_t)b * p.q_bs, k_boff = paged ? 0 : (int64_t)bkv * p.k_bs, v_boff = paged ? 0 : (int64_t)bkv * p.v_bs, o_boff = (int64_t)b * p.o_bs;
  if (VARLEN && p.cu_q) {  // varlen: rows cu[b] .. cu[b+1]-1  (reference block_info.h:17-36)
    const int c0 = p.cu_q[b];
    s.sq = p.cu_q[b + 1] - c0;
    s.q_row0 = c0;
    q_boff = 0;
    o_boff = 0;
  }
  if ((F & FB_SEQUSED) && p.seqused_q) s.sq = min(s.sq, p.seqused_q[b]);  // padded batch: only the first seqused_q[b] rows of the entry exist
  if (VARLEN && p.cu_k) {
    const int c0 = p.cu_k[b];
    s.sk = p.cu_k[b + 1] - c0;
    k_row0 = c0;
    k_boff = 0;
    v_boff = 0;
  }
  if (paged) k_row0 = 0;  // cu_seqlens_k gives a paged cache only the lengths
  // keys in use: never negative, never beyond the addressable capacity; inside a packed batch never beyond the entry's slot (as the backward: include/fa_gfx950.h)
  if ((F & (FB_SEQUSED | FB_CACHE)) && p.seqused_k)
    s.sk = max(0, min(p.seqused_k[b] + (CACHE ? p.seqused_add : 0), (VARLEN && p.cu_k && !paged) ? s.sk : p.sk));
  s.q_off = q_boff + s.q_row0 * p.q_rs;
  s.k_off = k_boff + k_row0 * p.k_rs;
  s.v_off = v_boff + k_row0 * p.v_rs;
  s.o_off = o_boff + s.q_row0 * p.o_rs;
  return s;
}
// log-sum-exp row of (b, head h): (h, total_q) in a packed batch, (b, h, sq) otherwise
template <int F> FA_DEVINL float* fwd_lse_row(const FwdK& p, const FwdSeq& s, int b, int h) {
  return ((F & FB_VARLEN) && p.cu_q) ? (p.lse + (int64_t)h * p.total_q + s.q_row0) : (p.lse + ((int64_t)b * p.h + h) * p.sq);
}

// ---- which keys a range of queries sees -------------------------------------------------------------------------------------------
// Query i sees keys max(0, i + shift - wl) .. min(sk - 1, i + shift + wr), shift = sk - sq (bottom-right alignment), a bound < 0 meaning
// "none" (reference mask.h:172-203; causal is wr = 0).  For queries q_first .. q_last that gives the keys some row sees -- tiles outside are
// skipped -- and the keys every row sees -- tiles inside need no mask.  all_lo is not clamped at 0: it is only compared against.
struct KeyWindow {
  int any_hi, any_lo;  // last / first key any row sees
  int all_hi, all_lo;  // keys <= all_hi and >= all_lo are visible to all rows
};
FA_DEVINL KeyWindow key_window(int q_first, int q_last, int shift, int sk, int wl, int wr) {
  KeyWindow w;
  w.any_hi = (wr >= 0) ? min(sk - 1, q_last + shift + wr) : sk - 1;
  w.any_lo = (wl >= 0) ? max(0, q_first + shift - wl) : 0;
  w.all_hi = (wr >= 0) ? min(sk - 1, q_first + shift + wr) : sk - 1;
  w.all_lo = (wl >= 0) ? (q_last + shift - wl) : 0;
  return w;
}

// 64-key tiles [n_min, n_min + n_tiles) a block scans: those its window touches (reference flash_fwd_kernel.h:90-94), cut to the share of key
// split `split` (may be empty)
struct TileRange {
  int n_min, n_tiles;
};
template <int F> FA_DEVINL TileRange tile_range(const FwdK& p, const KeyWindow& blk, int split) {
  constexpr int BN = 64;
  int n_min = blk.any_lo / BN;
  int n_max = (blk.any_hi >= blk.any_lo) ? (blk.any_hi / BN + 1) : n_min;
  if ((F & FB_SPLIT) && p.n_splits > 1) {
    n_min = max(n_min, split * p.split_tiles);
    n_max = max(n_min, min(n_max, (split + 1) * p.split_tiles));
  }
  return {n_min, n_max - n_min};
}

}  // namespace fa
