// Forward attention of FP8 (OCP e4m3) queries against an FP8 KV cache (fa_fwd_kvcache_fp8): the decode-side twin of fa_fwd_fp8.hip.
//
// Contract, operand maps, the transposed V image and the numerics are those of fa_fwd_fp8.hip (S = softmax_scale * q_descale * k_descale * q.k^T
// on the exact fp8 values, P rounded to e4m3, v_descale folded into 1 / l, deferred rescale capped at 8; probe_gfx950.hip checks the lane maps).
// What this kernel adds is the cache addressing and the decode schedule:
//   - keys in use per batch entry = seqused_k[b] + seqused_add, never more than the addressable capacity; rows past it are never read (a DMA lane
//     whose row lies behind the last key re-fetches the last key, and its score is masked);
//   - kv_batch_idx picks the cache row of a batch entry; the descales stay indexed by the batch entry of q;
//   - a paged cache resolves every 64-key tile through block_table (pages are multiples of 256 keys: a tile never straddles two pages);
//   - FwdK::pack_g = g > 1: the "head" is a KV head and its g * Sq rows are (query r / g, query head h * g + r % g), as fa_fwd_kernel defines it:
//     K / V stream once per KV head;
//   - n_splits > 1: the workgroup scans key tiles [split * split_tiles, (split + 1) * split_tiles) and writes a normalised fp32 partial O and its
//     log-sum-exp in the layout fa_splitkv_combine_kernel (fa_fwd.hip) reads; that kernel finishes the call with the bf16 output.
//
// Schedule.  An e4m3 tile is half the bytes of a bf16 one (64 keys x D bytes of K and as much of V) while the per-tile fixed cost (barrier, V image,
// two MFMA groups) is unchanged, so the two-slot ring of fa_fwd_fp8.hip would keep only 2 D x 64 bytes per workgroup in flight.  Here the K / V
// staging ring has NS slots and the LDS-DMA runs NS - 1 tiles ahead: iteration u issues tile u + NS - 1 into the slot tile u - 1 left, and waits
// with a COUNTED vmcnt -- only for its own pieces of tile u + 1 -- in front of a raw s_barrier (a __syncthreads() would drain the DMA in flight).
// Tile u + 1 is read in iteration u + 1, one barrier after the wait that retired it.  The V^T images stay double buffered.
// LDS: K[NS] | V[NS] | I0 | I1 (tile = 64 keys x D bytes; Q is staged in I0 | I1 before the loop, the epilogue stages O over the ring).
#include <cstdio>

#include "fa_device.h"
#include "fa_kernel_params.h"
#include "fa_launch.h"

namespace fa {

typedef __attribute__((ext_vector_type(8))) int i32x8;

namespace kv8 {
// D = A.B + C on e4m3 A and B (cbsz = blgp = 0), unit E8M0 block scales (127 = 2^0) on both operands
FA_DEVINL f32x16 mfma_e4m3(i32x8 a, i32x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
}
FA_DEVINL i32x8 join16(u32x4 lo, u32x4 hi) {
  return __builtin_bit_cast(i32x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// 16-byte chunk swizzles of the row tiles and of the V image: as fa_fwd_fp8.hip (every 16-lane group of a ds_read_b128 meets each 16-byte slot of
// a 256-byte bank row once)
template <int D> FA_DEVINL constexpr int swz_row8(int row) {
  return D == 128 ? (((row >> 1) & 1) | (((row >> 3) & 1) << 1) | (((row >> 2) & 1) << 2)) : ((row >> 2) & 3);
}
FA_DEVINL constexpr int swz_img(int d) { return (d >> 2) & 3; }
// at most N of this wave's LDS-DMA instructions still in flight (they retire in order)
template <int N> FA_DEVINL void dma_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// every LDS write and read of this wave done, then the workgroup barrier -- without the vmcnt(0) a __syncthreads() puts in front of it
FA_DEVINL void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
}  // namespace kv8

template <typename E, int D, int NS>
__global__ void __launch_bounds__(256, 2) fa_fwd_fp8_kv_kernel(const FwdK p, const Fp8K f8) {
  using namespace kv8;
  constexpr int NW = 4, BM = NW * 32, BN = 64;
  constexpr int ROW = D;                  // bytes per K / V / Q row
  constexpr int TILE = BN * ROW;          // bytes per K / V tile and per V image
  constexpr int CPR = D / 16;             // 16-byte chunks per row
  constexpr int KS = D / 64;              // MFMAs per 32-key half tile of S^T
  constexpr int DB = D / 32;              // 32-row blocks of O^T
  constexpr int PD = NS - 1;              // tiles the DMA runs ahead
  constexpr int K_OFF = 0, V_OFF = NS * TILE, I_OFF = 2 * NS * TILE;
  static_assert(D == 64 || D == 128, "head dims built: 64, 128");
  static_assert(NS >= 2 && NS <= 4, "ring depths built: 2, 3, 4");
  static_assert(sizeof(E) == 1, "one byte per element");
  constexpr float kLn2 = 0.6931471805599453f;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char FA_LDS* lds = (char FA_LDS*)smem;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, qi = lane & 31;

  // ---- which (batch, head, query block, key split): as fa_fwd_kernel ----
  const int w = xcd_interleave(blockIdx.x, p.n_units, p.unit_size, p.unit_hpx);
  if (w < 0) return;
  const int nmbs = p.nmb * p.n_splits;  // key splits of one query block are adjacent work items
  const int bh = w / nmbs;
  int mbr = w - bh * nmbs;
  const int split = __builtin_amdgcn_readfirstlane(mbr % p.n_splits);
  mbr /= p.n_splits;
  const int m_block = __builtin_amdgcn_readfirstlane((p.wr >= 0) ? (p.nmb - 1 - mbr) : mbr);
  const int b = __builtin_amdgcn_readfirstlane(bh / p.h);  // (the divisions run on the vector unit: back to scalar registers, so that the page table is read with scalar loads)
  const int h = __builtin_amdgcn_readfirstlane(bh) - b * p.h;
  const int hk = h / p.hk_ratio;

  const int sq = p.sq;
  int sk = p.sk;
  if (p.seqused_k) sk = max(0, min(p.seqused_k[b] + p.seqused_add, p.sk));  // keys in use, never beyond the addressable capacity
  const int bkv = p.kv_batch_idx ? p.kv_batch_idx[b] : b;  // cache row of this batch entry
  const int64_t k_boff = p.block_table ? 0 : (int64_t)bkv * p.k_bs, v_boff = p.block_table ? 0 : (int64_t)bkv * p.v_bs;  // paged: the page supplies it
  const int m0 = m_block * BM;
  if (m0 >= sq) return;

  const int g = p.pack_g;
  const bool packed = g > 1;
  auto q_of = [&](int row) __attribute__((always_inline)) { return packed ? row / g : row; };

  const char* __restrict__ qp = (const char*)p.q + (int64_t)b * p.q_bs + (int64_t)h * g * p.q_hs;
  const char* __restrict__ kp = (const char*)p.k + k_boff + (int64_t)hk * p.k_hs;
  const char* __restrict__ vp = (const char*)p.v + v_boff + (int64_t)hk * p.v_hs;
  __bf16* __restrict__ op = (__bf16*)p.o + (int64_t)b * p.o_bs + (int64_t)h * g * p.o_hs;
  float* __restrict__ lsep = p.lse + ((int64_t)b * p.h + h) * p.sq;  // packed: (b, h * g + r % g, r / g) == this base + (r % g) * (sq / g) + r / g

  // descales: per (batch entry of q, kv head) -- not per cache row
  const float qd = f8.q_descale ? f8.q_descale[(int64_t)b * f8.q_bs + (int64_t)hk * f8.q_hs] : 1.f;
  const float kd = f8.k_descale ? f8.k_descale[(int64_t)b * f8.k_bs + (int64_t)hk * f8.k_hs] : 1.f;
  const float vd = f8.v_descale ? f8.v_descale[(int64_t)b * f8.v_bs + (int64_t)hk * f8.v_hs] : 1.f;
  const float cs = p.scale_log2 * qd * kd;  // log2 units per unit of the raw fp8 dot product
  const float thr = p.rescale_thr;

  // ---- key range of the block and of this split, per-wave and per-lane visibility limits ----
  const int sq_true = packed ? sq / g : sq;
  const int shift = sk - sq_true;  // bottom-right alignment to this entry's own length
  const int blk_last = min(m0 + BM, sq) - 1;
  int kmax = sk - 1, kmin = 0;
  if (p.wr >= 0) kmax = min(kmax, q_of(blk_last) + shift + p.wr);
  if (p.wl >= 0) kmin = max(0, q_of(m0) + shift - p.wl);
  int n_min = kmin / BN;
  int n_max = (kmax >= kmin) ? (kmax / BN + 1) : n_min;
  if (p.n_splits > 1) {  // this workgroup's share of the key tiles (may be empty)
    n_min = max(n_min, split * p.split_tiles);
    n_max = max(n_min, min(n_max, (split + 1) * p.split_tiles));
  }
  const int n_tiles = n_max - n_min;
  const int key_base = n_min * BN;

  const int w_row0 = m0 + wave * 32;
  const int w_row1 = min(w_row0 + 31, sq - 1);
  const bool wave_valid = w_row0 < sq;
  const int w_q0 = q_of(w_row0), w_q1 = q_of(w_row1);
  const int w_kmax = (p.wr >= 0) ? min(sk - 1, w_q1 + shift + p.wr) : sk - 1;
  const int w_kmin = (p.wl >= 0) ? max(0, w_q0 + shift - p.wl) : 0;
  const int w_full_hi = (p.wr >= 0) ? min(sk - 1, w_q0 + shift + p.wr) : sk - 1;
  const int w_full_lo = (p.wl >= 0) ? (w_q1 + shift - p.wl) : 0;
  const int my_row = w_row0 + qi;
  const bool row_valid = my_row < sq;
  const int my_q = q_of(my_row);
  const int my_hh = my_row - my_q * g;  // head within the group (0 unless packed)
  const int lim_hi = (p.wr >= 0) ? min(sk - 1, my_q + shift + p.wr) : sk - 1;
  const int lim_lo = (p.wl >= 0) ? (my_q + shift - p.wl) : 0;

  // ---- K / V tiles global -> LDS by DMA (1 KiB per wave instruction, lane-linear destination; the swizzle is applied to the per-lane source
  // chunk).  Rows past the last key are clamped to the last key: bytes behind an entry's length are never read.
  constexpr int RPD = 1024 / ROW;        // tile rows per DMA instruction
  constexpr int DPW = TILE / 1024 / NW;  // DMA instructions per wave and tile (K and V each)
  constexpr int IPT = 2 * DPW;           // ... per wave and tile, K and V together
  static_assert(DPW >= 1 && (TILE / 1024) % NW == 0, "tile does not divide over the waves");
  static_assert(PD * IPT < 64, "the counted wait must fit vmcnt");
  const int d_row = lane / CPR, d_pc = lane % CPR;
  // first row of key tile n: contiguous cache row, or page block_table[b][n * 64 / page] of a paged cache.  The page indices are held one per lane,
  // 64 pages from pg_base on, and picked with v_readlane: a load inside the tile loop would be waited for with vmcnt(0) and drain the DMA ring
  // (the window is reloaded every 64 pages, >= 16k keys).
  const int32_t* __restrict__ bt = p.block_table ? p.block_table + (int64_t)b * p.block_table_bs : nullptr;
  const int n_pages = bt ? p.sk / p.page_size : 0;  // entries of a block_table row (paged: p.sk = entries * page_size)
  int pg_base = bt ? __builtin_amdgcn_readfirstlane((n_min * BN) / p.page_size) : 0;
  int pg_vec = bt ? bt[min(pg_base + lane, n_pages - 1)] : 0;
  asm volatile("" : "+v"(pg_vec));
  auto page_of = [&](int n) __attribute__((always_inline)) -> int {
    const int pg = __builtin_amdgcn_readfirstlane((n * BN) / p.page_size);
    if (pg - pg_base >= 64) {
      pg_base = pg;
      pg_vec = bt[min(pg_base + lane, n_pages - 1)];
      asm volatile("" : "+v"(pg_vec));  // the load is waited for here, inside the rare branch, not at the join every tile passes
    }
    return __builtin_amdgcn_readlane(pg_vec, pg - pg_base);
  };
  auto tile_row_off = [&](int n, int blk, int64_t bs, int64_t rs) __attribute__((always_inline)) -> int64_t {
    if (!bt) return (int64_t)n * BN * rs;
    const int key0 = n * BN;
    return (int64_t)blk * bs + (int64_t)(key0 - (key0 / p.page_size) * p.page_size) * rs;
  };
  auto dma_tile = [&](int slot, int t) __attribute__((always_inline)) {
    const int n = n_min + t;
    const int blk = bt ? page_of(n) : 0;
    const char* kbase = kp + tile_row_off(n, blk, p.k_bs, p.k_rs);
    const char* vbase = vp + tile_row_off(n, blk, p.v_bs, p.v_rs);
    char FA_LDS* kdst = lds + K_OFF + slot * TILE + wave * DPW * 1024;
    char FA_LDS* vdst = lds + V_OFF + slot * TILE + wave * DPW * 1024;
#pragma unroll
    for (int i = 0; i < DPW; ++i) {
      const int row = (wave * DPW + i) * RPD + d_row;
      const int grow = min(n * BN + row, sk - 1) - n * BN;
      const int ch = (d_pc ^ swz_row8<D>(row)) << 4;
      lds_dma_16B(kbase + (int64_t)grow * p.k_rs + ch, kdst + i * 1024);
      lds_dma_16B(vbase + (int64_t)grow * p.v_rs + ch, vdst + i * 1024);
    }
  };

  // Q block -> LDS (the two image buffers, unused until the loop) -> registers
  {
    constexpr int QDMA = BM * ROW / 1024 / NW;
#pragma unroll
    for (int i = 0; i < QDMA; ++i) {
      const int row = (wave * QDMA + i) * RPD + d_row;
      const int grow = min(m0 + row, sq - 1);
      const int gq = q_of(grow), ghh = grow - gq * g;
      lds_dma_16B(qp + (int64_t)gq * p.q_rs + (int64_t)(packed ? ghh : 0) * p.q_hs + ((d_pc ^ swz_row8<D>(row)) << 4), lds + I_OFF + (wave * QDMA + i) * 1024);
    }
  }
#pragma unroll
  for (int t = 0; t < PD; ++t)
    if (t < n_tiles) dma_tile(t, t);
  lds_dma_wait_all();
  lds_barrier();
  i32x8 qreg[KS];
  {
    const int row = wave * 32 + qi;
    const char FA_LDS* rb = lds + I_OFF + row * ROW;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int c = 4 * ks + 2 * hi;
      qreg[ks] = join16(*(const u32x4 FA_LDS*)(rb + ((c ^ swz_row8<D>(row)) << 4)), *(const u32x4 FA_LDS*)(rb + (((c + 1) ^ swz_row8<D>(row)) << 4)));
    }
  }
  lds_barrier();  // the image buffers are written from the first iteration on

  // ---- V tile -> V^T image (fa_fwd_fp8.hip): thread (kg, dg) moves keys 4 kg .. 4 kg + 3 x head-dim columns 8 dg .. 8 dg + 7
  constexpr int T_UNITS = 16 * (D / 8);
  const int t_kg = tid & 15, t_dg = tid >> 4;
  const int t_key0 = 4 * t_kg;
  const int t_chunk = 2 * (t_kg & 1) + (t_kg >> 3);  // logical 16-byte chunk of the image row that holds these 4 keys
  const int t_inoff = 4 * ((t_kg >> 1) & 3);         // byte offset inside that chunk
  auto transpose_v = [&](int slot, int img) __attribute__((always_inline)) {
    if (T_UNITS < NW * 64 && tid >= T_UNITS) return;
    const char FA_LDS* src = lds + V_OFF + slot * TILE;
    char FA_LDS* dst = lds + I_OFF + img * TILE;
    u32x2 r[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int row = t_key0 + t;
      const int lc = t_dg >> 1;  // logical 16-byte chunk of the 8 columns
      r[t] = *(const u32x2 FA_LDS*)(src + row * ROW + ((lc ^ swz_row8<D>(row)) << 4) + (t_dg & 1) * 8);
    }
#pragma unroll
    for (int ww = 0; ww < 2; ++ww) {  // columns 8 dg + 4 ww .. + 3
      const unsigned a = r[0][ww], bb = r[1][ww], c = r[2][ww], dd = r[3][ww];
      const unsigned t0 = __builtin_amdgcn_perm(bb, a, 0x05010400u);
      const unsigned t1 = __builtin_amdgcn_perm(bb, a, 0x07030602u);
      const unsigned t2 = __builtin_amdgcn_perm(dd, c, 0x05010400u);
      const unsigned t3 = __builtin_amdgcn_perm(dd, c, 0x07030602u);
      const unsigned o[4] = {__builtin_amdgcn_perm(t2, t0, 0x05040100u), __builtin_amdgcn_perm(t2, t0, 0x07060302u),
                             __builtin_amdgcn_perm(t3, t1, 0x05040100u), __builtin_amdgcn_perm(t3, t1, 0x07060302u)};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int d = 8 * t_dg + 4 * ww + e;
        *(unsigned FA_LDS*)(dst + d * 64 + ((t_chunk ^ swz_img(d)) << 4) + t_inoff) = o[e];
      }
    }
  };

  f32x16 o_acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[db][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  i32x8 pf = {0, 0, 0, 0, 0, 0, 0, 0};  // packed P^T of the previous tile (B operand)
  bool have_prev = false;

  // O^T += V^T.P^T from image `img`
  auto pv = [&](int img) __attribute__((always_inline)) {
    const char FA_LDS* im = lds + I_OFF + img * TILE;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const int d = 32 * db + qi;
      const char FA_LDS* rb = im + d * 64;
      const i32x8 vt = join16(*(const u32x4 FA_LDS*)(rb + (((2 * hi) ^ swz_img(d)) << 4)), *(const u32x4 FA_LDS*)(rb + (((2 * hi + 1) ^ swz_img(d)) << 4)));
      o_acc[db] = mfma_e4m3(vt, pf, o_acc[db]);
    }
  };
  // S^T of one 32-key half of the K tile in `slot`
  auto qk_half = [&](f32x16& s, int slot, int half) __attribute__((always_inline)) {
    const int row = 32 * half + qi;
    const char FA_LDS* rb = lds + K_OFF + slot * TILE + row * ROW;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int c = 4 * ks + 2 * hi;
      const i32x8 kf = join16(*(const u32x4 FA_LDS*)(rb + ((c ^ swz_row8<D>(row)) << 4)), *(const u32x4 FA_LDS*)(rb + (((c + 1) ^ swz_row8<D>(row)) << 4)));
      s = mfma_e4m3(kf, qreg[ks], s);
    }
  };
  auto apply_mask = [&](f32x16& s, int k0) __attribute__((always_inline)) {
    const int rel_hi = lim_hi - k0 - 4 * hi;
    const int rel_lo = lim_lo - k0 - 4 * hi;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int off = acc_row(r, 0);
      s[r] = ((off <= rel_hi) && (off >= rel_lo)) ? s[r] : -INFINITY;
    }
  };
  // registers 4g .. 4g+3 -> bytes 0 .. 3 of dword base + g
  auto pack = [&](const f32x16& s, int base) __attribute__((always_inline)) {
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
      int ww = __builtin_amdgcn_cvt_pk_fp8_f32(s[4 * gg], s[4 * gg + 1], 0, false);
      ww = __builtin_amdgcn_cvt_pk_fp8_f32(s[4 * gg + 2], s[4 * gg + 3], ww, true);
      pf[base + gg] = ww;
    }
  };

  int slot = 0, slot_pre = PD % NS;  // ring slots of tile u and of tile u + PD
  for (int u = 0; u < n_tiles; ++u) {
    const int img = u & 1;
    if (u + PD < n_tiles) dma_tile(slot_pre, u + PD);
    transpose_v(slot, img);
    if (have_prev) pv(img ^ 1);
    const int k0 = key_base + u * BN;
    const bool active = wave_valid && k0 <= w_kmax && k0 + BN - 1 >= w_kmin;
    if (active) {
      f32x16 sa, sb;
      qk_half(sa, slot, 0);
      qk_half(sb, slot, 1);
      if ((k0 + BN - 1 > w_full_hi) || (k0 < w_full_lo)) {
        apply_mask(sa, k0);
        apply_mask(sb, k0 + 32);
      }
      float tmax = fmaxf(sa[0], sb[0]);
#pragma unroll
      for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, fmaxf(sa[r], sb[r]));
      tmax = half_max(tmax);
      const float m_new = fmaxf(m_run, tmax);
      const bool grow = (m_new - m_run) * cs > thr;
      if (__any(grow)) {
        const float alpha = grow ? fast_exp2((m_run - m_new) * cs) : 1.f;
        if (grow) m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) o_acc[db][r] *= alpha;
      }
      const float neg_mc = (m_run == -INFINITY) ? 0.f : -m_run * cs;
      float ps0 = 0.f, ps1 = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sa[r] = fast_exp2(__builtin_fmaf(sa[r], cs, neg_mc));
        sb[r] = fast_exp2(__builtin_fmaf(sb[r], cs, neg_mc));
        ps0 += sa[r];
        ps1 += sb[r];
      }
      l_run += ps0 + ps1;
      pack(sa, 0);
      pack(sb, 4);
    }
    have_prev = active;
    // this wave's pieces of tile u + 1 have landed; later tiles stay in flight (the DMA retires in order)
    const int ahead = min(n_tiles - 2 - u, PD - 1);  // tiles issued behind tile u + 1
    if (PD >= 3 && ahead >= 2) dma_wait<(PD >= 3 ? 2 : 0) * IPT>();
    else if (PD >= 2 && ahead == 1) dma_wait<(PD >= 2 ? 1 : 0) * IPT>();
    else dma_wait<0>();
    lds_barrier();  // ... and everybody's pieces and image rows are visible
    slot = (slot + 1 == NS) ? 0 : slot + 1;
    slot_pre = (slot_pre + 1 == NS) ? 0 : slot_pre + 1;
  }
  if (have_prev) pv((n_tiles - 1) & 1);
  lds_barrier();  // every wave is done with the ring and the images before the epilogue stages O over them

  if (!wave_valid) return;
  const float l_tot = half_sum(l_run);
  const bool dead = (l_tot == 0.f) || (l_tot != l_tot);
  const float inv = dead ? 1.f : vd / l_tot;
  if (p.n_splits > 1) {  // partial result of this key split, fp32, merged by fa_splitkv_combine_kernel
    if (row_valid) {
      const int64_t prow = (((int64_t)split * p.b + b) * p.h + h) * p.sq + my_row;
      float* orow = p.o_accum + prow * D;
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
          f32x4 ov;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) ov[jj] = o_acc[db][4 * gg + jj] * inv;
          *reinterpret_cast<f32x4*>(orow + 32 * db + 8 * gg + 4 * hi) = ov;
        }
      if (hi == 0) p.lse_accum[prow] = dead ? -INFINITY : (m_run * cs * kLn2 + __logf(l_tot));
    }
    return;
  }
  char FA_LDS* stage = lds + wave * 32 * (2 * D + 16);
  if (packed) {
    store_tile_via_lds_packed<__bf16, D>(stage, o_acc, inv, op, p.o_rs, p.o_hs, g, w_row0, sq, lane);
    if (row_valid && hi == 0) lsep[(int64_t)my_hh * sq_true + my_q] = dead ? INFINITY : (m_run * cs * kLn2 + __logf(l_tot));
    return;
  }
  store_tile_via_lds<__bf16, D>(stage, o_acc, inv, op + (int64_t)w_row0 * p.o_rs, p.o_rs, sq - w_row0, lane);
  if (row_valid && hi == 0) lsep[my_row] = dead ? INFINITY : (m_run * cs * kLn2 + __logf(l_tot));
}

struct e4m3 { unsigned char bits; };  // element tag of the kernel's name

template <int D, int NS>
static int launch_fwd_fp8_kv_t(const FwdK& p, const Fp8K& f8, hipStream_t stream) {
  constexpr int smem = (2 * NS + 2) * 64 * D;
  static_assert(4 * 32 * (2 * D + 16) <= smem, "epilogue staging does not fit");
  auto kern = fa_fwd_fp8_kv_kernel<e4m3, D, NS>;
  static std::atomic<unsigned long long> attr_mask{0};  // LDS is addressed by byte offset: the dynamic segment must start at 0
  if (ensure_dyn_lds(attr_mask, (const void*)kern, smem, true) != 0) return -1;
  const long long total = units_grid(p.n_units, p.unit_size);
  if (total <= 0) return 0;
  hipLaunchKernelGGL(kern, dim3((unsigned)total), dim3(256), smem, stream, p, f8);
  if (hipGetLastError() != hipSuccess) return -1;
  LastSchedule& ls = last_schedule();
  ls.fwd_kernel = 5; ls.fwd_nw = 4; ls.fwd_feat = 0; ls.fwd_splits = p.n_splits; ls.fwd_list = 0; ls.d = D;
  ls.bf16 = 0; ls.fwd_pack = p.pack_g;
  snprintf(ls.name, sizeof(ls.name), "fa::fa_fwd_fp8_kv_kernel<e4m3,%d,ring%d>", D, NS);
  return 0;
}

template <int D>
static int launch_fwd_fp8_kv_d(const FwdK& p, const Fp8K& f8, int ring, hipStream_t stream) {
  if (ring == 2) return launch_fwd_fp8_kv_t<D, 2>(p, f8, stream);
  if (ring == 3) return launch_fwd_fp8_kv_t<D, 3>(p, f8, stream);
  return launch_fwd_fp8_kv_t<D, 4>(p, f8, stream);
}

int launch_fwd_fp8_kv(const FwdK& p, const Fp8K& f8, int d, hipStream_t stream) {
  if ((uint64_t)64 * (uint64_t)(p.k_rs > p.v_rs ? p.k_rs : p.v_rs) >= (1ull << 31)) return -3;
  const int ring = knobs().fp8_kv_ring;
  if (d == 128) return launch_fwd_fp8_kv_d<128>(p, f8, ring, stream);
  if (d == 64) return launch_fwd_fp8_kv_d<64>(p, f8, ring, stream);
  return -2;
}

}  // namespace fa
