// Absorbed multi-head latent attention (MLA) decode against a KV cache, gfx950 (MI355X): q / k head dim 576 (512 latent + 64 rotary channels), v / o head
// dim 512, and V IS the first 512 channels of the K row -- one cache row per key, one shared KV head in the real workload (DeepSeek-V2/V3 decode; the
// published FlashMLA shape, "Q/K <= 64 with V <= 512 plus qv" in the reference's newer interface).  fa_fwd_kvcache only (fa_api.cpp refuses the rest).
//
// Orientation, tile feed, masks and the "no visible key => out = 0, lse = +inf" rule are those of fa_fwd_dv.hip / fa_fwd_fp8_kv.hip: S^T = K.Q^T on
// v_mfma_f32_32x32x16 with the query on the lane, lane-local online softmax in fp32 (every score scaled in fp32), O^T += V^T.P^T with the key
// permutation applied to the transposed LDS reads, K tiles by LDS-DMA into a two-slot ring, block geometry from fa_fwd_block.h
// (FB_CACHE | FB_SPLIT | FB_SCALAR).  What is new: ONE LDS image of a 64-key tile serves both products.  The K fragments are ds_read_b128 reads of all
// 576 channels; the V^T fragments are ds_read_b64_tr_b16 reads of channels 0 .. 511 of the same image; channels 512 .. 575 are never read on the
// value side.  Every cache row is fetched from HBM once.
//
// Rows.  Always the packed layout of fa_fwd_kernel (FwdK::pack_g = g = H / Hk >= 1): the "head" is a KV head, row r of its g * Sq rows is query r / g
// of query head head * g + r % g, and there are as many 64-row query blocks as g * Sq needs -- the cache streams once per 64 rows, not once per head.
//
// Schedule (the form built, and why).  A 64-key tile is 64 x 1152 B = 72 KB; two slots are 144 KB of the CU's 160 KB: one 4-wave workgroup per CU,
// the whole 512-register file per lane.  "Every wave owns 32 rows and all 512 channels" needs 144 (Q) + 256 (O^T) + 32 (S) = 432 registers before any
// fragment or address: too tight for compiler-scheduled code.  Built instead: a 64-row block whose wave (qh, ch) owns the 32 rows of query half qh
// and the 256 value channels of channel half ch.  Both waves of a query half compute the same 64-key x 32-query score block (72 MFMAs each, the
// duplicate is the price) and the same lane-local softmax, so nothing is exchanged through LDS and a tile costs ONE barrier; each then accumulates its
// own 8 output blocks (32 MFMAs).
//   per wave and tile (arithmetic): 104 MFMAs = 3 328 MFMA clocks at 32 clocks each; 72 ds_read_b128 (72 KB) + 64 ds_read_b64_tr_b16 (32 KB), four
//     waves = 416 KB = 3 250 clocks of LDS at 128 B / clock; about 180 vector instructions for the tile feed (18 pieces x ~10: the walk, the swizzle, one
//     32-bit multiply; the DMA takes a scalar base and a 32-bit lane offset) and about 360 for mask and softmax.  With one wave per SIMD none of these
//     hides another.  A CU has ~5 000 clocks per 72 KB tile at the chip's HBM rate.
//   measured (profiles/fwd_mla_decode.txt): ~4.9 us per tile and workgroup at H = 16 (14.4 - 14.9 GB/s of cache per workgroup whatever the batch), so the
//     kernel is bound by its own tile loop, not by HBM; the chip's rate (3.8 TB/s at B = 64) needs all 256 CUs occupied.  From two blocks per KV head on
//     (H = 128) it is MFMA-bound and the duplicated scores cost 104 / 68 of the exchanging form.
//   registers (arithmetic): Q as B operand 36 k-steps x 4 = 144, O^T 8 blocks x 16 = 128, S 32, P^T 16, K fragments 3 x 8 = 24, V^T fragments 16;
//   as built: see profiles/fwd_mla_resource_usage.txt (256 VGPR + 235 AGPR, no scratch, no spill).
//
// Swizzle for the 1152-byte row.  1152 = 4.5 x 256: row r starts at 16-byte slot 8 * (r & 1) of a 256-byte bank row, as a 128-byte pitch does.
// The low three bits of a 16-byte chunk index c are XORed with f(r) = bits (0, 1, 2) of (r >> 1) & 7 taken in the order (2, 1, 0); the XOR never
// leaves the 8-chunk group, so chunk c < 72 stays inside the row.
//   K (ds_read_b128, lane = key row, all lanes the same chunk): the 16 lanes served together hold 8 even and 8 odd rows whose (r >> 1) & 7 takes every
//     value once per parity (fa_fwd_dv.hip) -- f is a bijection, so the 8 rows of a parity land on 8 different slots of their half: conflict-free.
//   V^T (ds_read_b64_tr_b16, a half-wave reads rows 4 hi + (0..3) (+ 8 b + 16 kk), 32 B of each per 16-lane group, two groups): row 4 hi + rr has
//     f = 4 (rr >> 1) + 2 hi + b, so rows rr = 0 / 2 (same parity, same half of the bank row) differ in chunk bit 2 and rows rr = 1 / 3 likewise: the
//     four rows cover slots {0-3, 8-11, 4-7, 12-15} (+ constants), the two groups and the two chunks of a 32-byte piece are distinct inside a 4-slot
//     set, the 8-byte halves inside a slot: 32 lanes x 8 B = all 64 banks once.  Conflict-free as well (by arithmetic; not measured with counters).
#include <cstdio>
#include <type_traits>

#include "fa_device.h"
#include "fa_fwd_block.h"
#include "fa_kernel_params.h"
#include "fa_launch.h"

namespace fa {

FA_DEVINL constexpr int mla_swz(int row) {  // K-image rows, low three bits of the 16-byte chunk index
  const int x = (row >> 1) & 7;
  return ((x & 1) << 2) | (x & 2) | (x >> 2);
}

// LDS-DMA of 16 bytes per lane from a wave-uniform base plus a 32-bit per-lane byte offset (fa_device.h lds_dma_16B with the scalar-base addressing
// form: no 64-bit address arithmetic per lane); destination = wave-uniform LDS byte address + 16 * lane.  Waited for with lds_dma_wait_all().
FA_DEVINL void lds_dma_16B_s(const void* base_uniform, unsigned lane_off, unsigned lds_dst_uniform) {
  const unsigned long long sb = (unsigned long long)base_uniform;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)sb), hi = __builtin_amdgcn_readfirstlane((unsigned)(sb >> 32));
  const unsigned long long base = ((unsigned long long)hi << 32) | lo;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_dst_uniform);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(lane_off), "s"(base), "s"(dst)
               : "memory");
}

template <int N> using ICmla = std::integral_constant<int, N>;

template <typename E, int DQK, int DV, int NW>
__global__ void __launch_bounds__(NW * 64, 1) fa_fwd_mla_kernel(const FwdK p) {
  using T = ElemTraits<E>;
  using V8 = typename T::v8;
  using V4 = typename T::v4;
  constexpr int BM = 64, BN = 64;
  constexpr int KCPR = DQK / 8;            // 16-byte chunks per row: 72
  constexpr int KROW = DQK * 2;            // row pitch of the tile image: 1152 B
  constexpr int KT = BN * KROW;            // 72 KB
  constexpr int KS = DQK / 16;             // 36 k-steps of S^T
  constexpr int CW = DV / 2;               // value channels per wave: 256
  constexpr int DB = CW / 32;              // 8 output blocks per wave
  constexpr int DPW = KT / 1024 / NW;      // LDS-DMA instructions per wave and tile: 18
  static_assert(DQK == 576 && DV == 512 && NW == 4, "swizzle, pitch and the wave roles are derived for (576, 512) and four waves");
  static_assert(KT % (1024 * NW) == 0 && 2 * KT <= 160 * 1024, "two tile slots, one workgroup per CU");
  static_assert(3 * 16 * KROW + (DB / 2 - 1) * 128 < 65536, "the transposed reads' immediates must fit a 16-bit LDS offset");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char FA_LDS* lds = (char FA_LDS*)smem;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qh = wave & 1, ch = wave >> 1;   // query half / channel half of this wave
  const int hi = lane >> 5, qi = lane & 31;

  // the host contract: no varlen, no work list, no seqused_q, no leftpad_k
  constexpr int F = FB_CACHE | FB_SPLIT | FB_SCALAR;
  FwdWork wk;
  if (!fwd_work<F>(p, blockIdx.x, wk)) return;
  const int b = wk.b, h = wk.h, split = wk.split;   // h: KV head (rows are packed)
  const FwdSeq seq = fwd_seq<F>(p, b);
  const int sq = seq.sq, sk = seq.sk;               // sq: packed rows; sk: keys in use of this entry's cache row
  const int m0 = wk.m_block * BM;
  if (m0 >= sq) return;

  const int g = p.pack_g;
  auto q_of = [&](int row) __attribute__((always_inline)) { return g > 1 ? row / g : row; };

  const E* __restrict__ qp = (const E*)p.q + seq.q_off + (int64_t)h * g * p.q_hs;
  const E* __restrict__ kp = (const E*)p.k + seq.k_off + (int64_t)h * p.k_hs;
  E* __restrict__ op = (E*)p.o + seq.o_off + (int64_t)h * g * p.o_hs;
  float* __restrict__ lsep = fwd_lse_row<F>(p, seq, b, h);  // (b, h * g + r % g, r / g) == this base + (r % g) * (sq / g) + r / g

  // ---- key tiles of the block and of this split, visibility limits of this wave's 32 rows and of this lane's row ----
  const int sq_true = sq / g;
  const int shift = sk - sq_true;  // bottom-right alignment to this entry's own length
  const TileRange tr = tile_range<F>(p, key_window(q_of(m0), q_of(min(m0 + BM, sq) - 1), shift, sk, p.wl, p.wr), split);
  const int n_min = tr.n_min, n_tiles = tr.n_tiles;
  const int w_row0 = m0 + qh * 32, my_row = w_row0 + qi;
  const bool wave_valid = w_row0 < sq, row_valid = my_row < sq;
  const int my_q = q_of(my_row);
  const int my_hh = my_row - my_q * g;  // head within the group
  const KeyWindow wv = key_window(q_of(w_row0), q_of(min(w_row0 + 31, sq - 1)), shift, sk, p.wl, p.wr);
  const KeyWindow ln = key_window(my_q, my_q, shift, sk, p.wl, p.wr);
  const float cs = p.scale_log2;
  const float thr = p.rescale_thr;

  // ---- Q fragments (B operand of S^T = K.Q^T): lane = packed row, 8 consecutive channels per k-step, 16-byte loads at row / head stride ----
  V8 qf[KS];
  {
    const E* qrow = qp + (int64_t)my_q * p.q_rs + (int64_t)my_hh * p.q_hs + 8 * hi;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = bitcast_u32x4<V8>(ld_global_16B(qrow + 16 * ks, row_valid));
  }

  // ---- tile feed: 1 KiB per wave instruction, lane-linear destination, so piece pi of a tile holds the 16-byte positions 64 * pi + lane;
  // position L is (row L / 72, chunk position L % 72) and fetches the SOURCE chunk the swizzle assigns to it.  A DMA lane past the last key
  // re-fetches the last key (its score is masked): bytes behind an entry's length are never read.  A paged cache resolves every tile through
  // block_table (pages are multiples of 256 keys: a tile never straddles two pages).  The page indices are held one per lane, 64 pages from
  // pg_base on, and picked with v_readlane, as in fa_fwd_fp8_kv.hip: behind the DMA's asm the compiler reads the table with a vector load and
  // waits for it with vmcnt(0), i.e. for the tile in flight (the window is reloaded every 64 pages, >= 16k keys). ----
  const int32_t* __restrict__ bt = p.block_table ? p.block_table + (int64_t)b * p.block_table_bs : nullptr;
  const int n_pages = bt ? p.sk / p.page_size : 0;  // entries of a block_table row (paged: p.sk = entries * page_size)
  int pg_base = bt ? __builtin_amdgcn_readfirstlane((n_min * BN) / p.page_size) : 0;
  int pg_vec = bt ? bt[min(pg_base + lane, n_pages - 1)] : 0;
  asm volatile("" : "+v"(pg_vec));
  const unsigned rs_bytes = (unsigned)p.k_rs * 2u;  // (host: a 64-key tile spans < 2 GiB, so a lane's offset from the tile's first row fits 32 bits)
  auto dma_tile = [&](int buf, int n) __attribute__((always_inline)) {
    const int key0 = n * BN;
    int64_t toff = (int64_t)key0 * p.k_rs;
    if (bt) {
      const int pg = __builtin_amdgcn_readfirstlane(key0 / p.page_size);
      if (pg - pg_base >= 64) {
        pg_base = pg;
        pg_vec = bt[min(pg_base + lane, n_pages - 1)];
        asm volatile("" : "+v"(pg_vec));  // the load is waited for here, inside the rare branch
      }
      const int blk = __builtin_amdgcn_readlane(pg_vec, pg - pg_base);
      toff = (int64_t)blk * p.k_bs + (int64_t)(key0 - pg * p.page_size) * p.k_rs;
    }
    const E* base = kp + toff;                 // wave-uniform: the DMA takes it as its scalar base, the lane supplies a 32-bit byte offset
    const int last = sk - 1 - key0;            // last row of the tile that is a key (>= 0)
    const unsigned dst = (unsigned)(unsigned long long)(lds + buf * KT + wave * DPW * 1024);
    // this wave's first piece starts at row 16 * wave, position `lane` (18 pieces = 16 rows); a piece later the position is 64 further.  The walk is
    // redone for every tile (the empty asm keeps the 18 (row, position) pairs from being hoisted into registers the accumulators need):
    // about 10 vector instructions per piece
    int row = wave * (DPW * 64 / KCPR), pc = lane;
    asm volatile("" : "+v"(pc));
#pragma unroll
    for (int i = 0; i < DPW; ++i) {
      const unsigned off = (unsigned)min(row, last) * rs_bytes + (unsigned)((pc ^ mla_swz(row)) << 4);
      lds_dma_16B_s(base, off, dst + i * 1024);
      const bool wrap = pc >= KCPR - 64;
      pc += wrap ? 64 - KCPR : 64;
      row += wrap ? 1 : 0;
    }
  };

  // ---- per-lane LDS read addresses (loop invariant; slots, k-steps past the swizzled 8-chunk group, key blocks and output blocks are immediates) ----
  int kaddr[4];   // k-step ks reads chunk 2 ks + hi = 8 * (ks >> 2) + (2 * (ks & 3) + hi): only the low three bits are swizzled
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) kaddr[k4] = qi * KROW + (((2 * k4 + hi) ^ mla_swz(qi)) << 4);
  // transposed reads: lane i of a 16-lane group addresses key row (i >> 2), channels 4 (i & 3) .. + 3 of a 4 x 16 block; group (lane >> 4) & 1 takes
  // the second 16 channels of the 32-channel output block; half-wave hi takes keys 4 hi .. + 3 (+ 8 for the fragment's upper half)
  const int tr_i = lane & 15, tr_half = (lane >> 4) & 1;
  const int tr_rr = tr_i >> 2, tr_cc = tr_i & 3;
  int vaddr[2][2];   // [upper half of the fragment: key + 8][output block parity]; chunk = 32 ch + 4 db + 2 tr_half + (tr_cc >> 1), f(row) = 4 (rr >> 1) + 2 hi + b
#pragma unroll
  for (int ub = 0; ub < 2; ++ub)
#pragma unroll
    for (int dp = 0; dp < 2; ++dp) {
      const int row = 8 * ub + 4 * hi + tr_rr;
      const int c3 = ((dp << 2) | (tr_half << 1) | (tr_cc >> 1)) ^ mla_swz(row);
      vaddr[ub][dp] = row * KROW + ch * (CW * 2) + (c3 << 4) + (tr_cc & 1) * 8;
    }

  // ---- online-softmax state (per lane = per packed row; both half-waves, and both waves of a query half, keep identical m) ----------
  f32x16 o_acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[db][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  f32x16 s[2];
  V8 pf[4];

  auto tile_active = [&](int j) __attribute__((always_inline)) {  // j relative to n_min
    const int kv0 = (n_min + j) * BN;
    return wave_valid && (kv0 <= wv.any_hi) && (kv0 + BN - 1 >= wv.any_lo);
  };

  // S^T[key][row] of the tile in slot `buf`: 36 k-steps x 2 key blocks; operand reads run PF k-steps ahead of their MFMAs
  auto qk = [&](auto bufc) __attribute__((always_inline)) {
    constexpr int buf = decltype(bufc)::value;
    const char FA_LDS* kbuf = lds + buf * KT;
    constexpr int PF = 3;
    u32x4 kfrag[PF][2];
    auto rd = [&](int ks) __attribute__((always_inline)) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) kfrag[ks % PF][kb] = *(const u32x4 FA_LDS*)(kbuf + kaddr[ks & 3] + (ks >> 2) * 128 + kb * 32 * KROW);
    };
#pragma unroll
    for (int ks = 0; ks < PF - 1; ++ks) rd(ks);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + PF - 1 < KS) rd(ks + PF - 1);
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch above this step's MFMAs
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        f32x16 c = s[kb];
        if (ks == 0) {
#pragma unroll
          for (int r = 0; r < 16; ++r) c[r] = 0.f;
        }
        s[kb] = T::mfma(bitcast_u32x4<V8>(kfrag[ks % PF][kb]), qf[ks], c);
      }
    }
  };

  // mask + online softmax of s -> pf (P^T as B operand), updates m_run / l_run / o_acc scale (fa_fwd_dv_kernel's rule)
  auto softmax_step = [&](int j) __attribute__((always_inline)) {
    const int kv0 = (n_min + j) * BN;
    const bool need_mask = (kv0 + BN - 1 > wv.all_hi) || (kv0 < wv.all_lo);
    if (need_mask) {
      const int rel_hi = ln.all_hi - kv0 - 4 * hi;
      const int rel_lo = ln.all_lo - kv0 - 4 * hi;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int off = 32 * kb + acc_row(r, 0);
          const bool vis = (off <= rel_hi) && (off >= rel_lo);
          s[kb][r] = vis ? s[kb][r] : -INFINITY;
        }
    }
    float tmax = s[0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, s[0][r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[1][r]);
    tmax = half_max(tmax);

    const float m_new = fmaxf(m_run, tmax);
    const bool grow = (m_new - m_run) * cs > thr;  // first visible key: -inf -> finite is always "grow"
    if (__any(grow)) {
      const float m_upd = grow ? m_new : m_run;
      const float m_safe = (m_upd == -INFINITY) ? 0.f : m_upd;
      const float alpha = grow ? fast_exp2((m_run - m_safe) * cs) : 1.f;
      m_run = m_upd;
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[db][r] *= alpha;
    }
    const float neg_mc = (m_run == -INFINITY) ? 0.f : -m_run * cs;  // fully masked so far
    float psum0 = 0.f, psum1 = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const float p0 = fast_exp2(__builtin_fmaf(s[kb][r], cs, neg_mc));
        const float p1 = fast_exp2(__builtin_fmaf(s[kb][r + 1], cs, neg_mc));
        s[kb][r] = p0;
        s[kb][r + 1] = p1;
        psum0 += p0;
        psum1 += p1;
      }
    l_run += psum0 + psum1;
    // P^T as B operand: k-step (kb,t) <-> accumulator registers 8t..8t+7 of s[kb]
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) pf[kb * 2 + t][jj] = (E)s[kb][8 * t + jj];
  };

  // O^T[d][row] += V^T[d][key] . P^T[key][row] over this wave's 256 channels: 4 key groups x 8 output blocks, read from the SAME image the scores
  // came from; transposed reads run PFV MFMAs ahead
  auto pv = [&](auto bufc) __attribute__((always_inline)) {
    constexpr int buf = decltype(bufc)::value;
    const char FA_LDS* vbuf = lds + buf * KT;
    constexpr int NOP = 4 * DB, PFV = 4;
    s16x4 vlo[PFV], vhi[PFV];
    auto rd = [&](int i) __attribute__((always_inline)) {
      const int db = i % DB, kk = i / DB;
      vlo[i % PFV] = lds_read_tr16(vbuf + vaddr[0][db & 1] + (db >> 1) * 128 + 16 * kk * KROW);
      vhi[i % PFV] = lds_read_tr16(vbuf + vaddr[1][db & 1] + (db >> 1) * 128 + 16 * kk * KROW);
    };
#pragma unroll
    for (int i = 0; i < PFV - 1; ++i) rd(i);
#pragma unroll
    for (int i = 0; i < NOP; ++i) {
      if (i + PFV - 1 < NOP) rd(i + PFV - 1);
      __builtin_amdgcn_sched_barrier(0);
      o_acc[i % DB] = T::mfma(combine_tr<V8>(vlo[i % PFV], vhi[i % PFV]), pf[i / DB], o_acc[i % DB]);
    }
  };

  // ---- lock-step key loop: per tile {DMA the next tile into the other slot, QK^T, softmax, PV, wait, barrier} ----
  if (n_tiles > 0) {
    dma_tile(0, n_min);
    lds_dma_wait_all();
    __syncthreads();
  }
  auto step = [&](auto bufc, int j) __attribute__((always_inline)) {
    constexpr int buf = decltype(bufc)::value;
    if (j + 1 < n_tiles) dma_tile(buf ^ 1, n_min + j + 1);  // lands in the other slot while this tile is being computed
    if (tile_active(j)) {
      qk(bufc);
      softmax_step(j);
      pv(bufc);
    }
    lds_dma_wait_all();  // this wave's pieces have landed ...
    __syncthreads();     // ... and everybody's are visible before the next tile reads them
  };
  for (int j = 0; j < n_tiles; j += 2) {
    step(ICmla<0>{}, j);
    if (j + 1 < n_tiles) step(ICmla<1>{}, j + 1);
  }

  // ---- epilogue: normalise; every lane holds groups of 4 consecutive channels of its row (32 db + 8 gq + 4 hi), stored directly ----
  if (!row_valid) return;
  const float l_tot = half_sum(l_run);
  const bool dead = (l_tot == 0.f) || (l_tot != l_tot);  // no visible key: out = 0, lse = +inf
  const float inv = dead ? 1.f : 1.f / l_tot;
  const float lse = m_run * p.scale + __logf(l_tot);
  const int c0 = ch * CW + 4 * hi;
  if (p.n_splits > 1) {  // partial result of this key split, fp32 rows of DV, merged by fa_splitkv_combine_kernel
    const int64_t prow = (((int64_t)split * p.b + b) * p.h + h) * p.sq + my_row;
    float* orow = p.o_accum + prow * DV + c0;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        f32x4 ov;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) ov[jj] = o_acc[db][4 * gq + jj] * inv;
        *reinterpret_cast<f32x4*>(orow + 32 * db + 8 * gq) = ov;
      }
    if (hi == 0 && ch == 0) p.lse_accum[prow] = dead ? -INFINITY : lse;
    return;
  }
  E* orow = op + (int64_t)my_q * p.o_rs + (int64_t)my_hh * p.o_hs + c0;
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      V4 ov;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) ov[jj] = (E)(o_acc[db][4 * gq + jj] * inv);
      *reinterpret_cast<V4*>(orow + 32 * db + 8 * gq) = ov;
    }
  if (hi == 0 && ch == 0) lsep[(int64_t)my_hh * sq_true + my_q] = dead ? INFINITY : lse;
}

template <typename E>
static int launch_fwd_mla_e(const FwdK& p, hipStream_t stream) {
  constexpr int NW = 4, DQK = 576, DV = 512;
  constexpr int smem = 2 * 64 * DQK * 2;   // 144 KB: two slots of one 64-key tile image
  auto kern = fa_fwd_mla_kernel<E, DQK, DV, NW>;
  static std::atomic<unsigned long long> attr_mask{0};
  if (ensure_dyn_lds(attr_mask, (const void*)kern, smem) != 0) return -1;
  const long long total = units_grid(p.n_units, p.unit_size);
  if (total <= 0) return 0;
  FA_LAUNCH(kern, dim3((unsigned)total), dim3(NW * 64), smem, stream, p);
  if (hipGetLastError() != hipSuccess) return -1;
  LastSchedule& ls = last_schedule();
  ls.fwd_kernel = 7; ls.fwd_nw = NW; ls.fwd_feat = FEAT_NONE; ls.fwd_splits = p.n_splits; ls.fwd_list = 0; ls.d = DQK; ls.dv = DV; ls.fwd_pack = p.pack_g;
  ls.bf16 = std::is_same<E, __bf16>::value;
  snprintf(ls.name, sizeof(ls.name), "fa::fa_fwd_mla_kernel<%s,%d,%d,%d>", ls.bf16 ? "bf16" : "f16", DQK, DV, NW);
  return 0;
}

int launch_fwd_mla(const FwdK& p, int dtype_bf16, int d, int dv, hipStream_t stream) {
  if (d != 576 || dv != 512) return -2;
  if ((uint64_t)64 * (uint64_t)p.k_rs * 2u >= (1ull << 31)) return -3;   // a lane's byte offset inside a 64-key tile is 32 bits wide
  return dtype_bf16 ? launch_fwd_mla_e<__bf16>(p, stream) : launch_fwd_mla_e<_Float16>(p, stream);
}

}  // namespace fa
