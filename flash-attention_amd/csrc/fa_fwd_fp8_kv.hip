// Forward attention of FP8 (OCP e4m3) queries against an FP8 KV cache (fa_fwd_kvcache_fp8): the decode-side twin of fa_fwd_fp8.hip.
//
// Contract, operand maps, the transposed V image and the numerics are those of fa_fwd_fp8.hip: both kernels take their tile code from fa_fp8_tile.h,
// where they are written down, and their block geometry from fa_fwd_block.h.
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
#include "fa_fp8_tile.h"
#include "fa_fwd_block.h"
#include "fa_kernel_params.h"
#include "fa_launch.h"

namespace fa {

template <typename E, int D, int NS>
__global__ void __launch_bounds__(256, 2) fa_fwd_fp8_kv_kernel(const FwdK p, const Fp8K f8) {
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

  // the host contract: no varlen, no work list, no seqused_q, no leftpad_k
  constexpr int F = FB_CACHE | FB_SPLIT | FB_SCALAR;
  FwdWork wk;
  if (!fwd_work<F>(p, blockIdx.x, wk)) return;
  const int b = wk.b, h = wk.h, split = wk.split, hk = h / p.hk_ratio;
  const FwdSeq seq = fwd_seq<F>(p, b);
  const int sq = seq.sq, sk = seq.sk;  // sk: keys in use of this entry's cache row
  const int m0 = wk.m_block * BM;
  if (m0 >= sq) return;

  const int g = p.pack_g;
  const bool packed = g > 1;
  auto q_of = [&](int row) __attribute__((always_inline)) { return packed ? row / g : row; };

  const char* __restrict__ qp = (const char*)p.q + seq.q_off + (int64_t)h * g * p.q_hs;
  const char* __restrict__ kp = (const char*)p.k + seq.k_off + (int64_t)hk * p.k_hs;
  const char* __restrict__ vp = (const char*)p.v + seq.v_off + (int64_t)hk * p.v_hs;
  __bf16* __restrict__ op = (__bf16*)p.o + seq.o_off + (int64_t)h * g * p.o_hs;
  float* __restrict__ lsep = fwd_lse_row<F>(p, seq, b, h);  // packed: (b, h * g + r % g, r / g) == this base + (r % g) * (sq / g) + r / g

  // descales: per (batch entry of q, kv head) -- not per cache row
  const float qd = f8.q_descale ? f8.q_descale[(int64_t)b * f8.q_bs + (int64_t)hk * f8.q_hs] : 1.f;
  const float kd = f8.k_descale ? f8.k_descale[(int64_t)b * f8.k_bs + (int64_t)hk * f8.k_hs] : 1.f;
  const float vd = f8.v_descale ? f8.v_descale[(int64_t)b * f8.v_bs + (int64_t)hk * f8.v_hs] : 1.f;
  const float cs = p.scale_log2 * qd * kd;  // log2 units per unit of the raw fp8 dot product
  const float thr = p.rescale_thr;

  // ---- key tiles of the block and of this split, visibility limits of this wave's 32 rows and of this lane's row ----
  const int sq_true = packed ? sq / g : sq;
  const int shift = sk - sq_true;  // bottom-right alignment to this entry's own length
  const TileRange tr = tile_range<F>(p, key_window(q_of(m0), q_of(min(m0 + BM, sq) - 1), shift, sk, p.wl, p.wr), split);
  const int n_min = tr.n_min, n_tiles = tr.n_tiles, key_base = n_min * BN;
  const int w_row0 = m0 + wave * 32, my_row = w_row0 + qi;
  const bool wave_valid = w_row0 < sq, row_valid = my_row < sq;
  const int my_q = q_of(my_row);
  const int my_hh = my_row - my_q * g;  // head within the group (0 unless packed)
  const KeyWindow wv = key_window(q_of(w_row0), q_of(min(w_row0 + 31, sq - 1)), shift, sk, p.wl, p.wr);
  const KeyWindow ln = key_window(my_q, my_q, shift, sk, p.wl, p.wr);

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
  fp8_read_q<D>(qreg, lds + I_OFF, wave * 32 + qi, hi);
  lds_barrier();  // the image buffers are written from the first iteration on

  f32x16 o_acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[db][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  i32x8 pf = {0, 0, 0, 0, 0, 0, 0, 0};  // packed P^T of the previous tile (B operand)
  bool have_prev = false;

  int slot = 0, slot_pre = PD % NS;  // ring slots of tile u and of tile u + PD
  for (int u = 0; u < n_tiles; ++u) {
    const int img = u & 1;
    if (u + PD < n_tiles) dma_tile(slot_pre, u + PD);
    fp8_transpose_v<D, NW * 64>(lds + V_OFF + slot * TILE, lds + I_OFF + img * TILE, tid);
    if (have_prev) fp8_pv<D>(o_acc, lds + I_OFF + (img ^ 1) * TILE, pf, qi, hi);
    const int k0 = key_base + u * BN;
    const bool active = wave_valid && k0 <= wv.any_hi && k0 + BN - 1 >= wv.any_lo;
    if (active) {
      f32x16 sa, sb;
      fp8_qk_half<D>(sa, lds + K_OFF + slot * TILE, qreg, 0, qi, hi);
      fp8_qk_half<D>(sb, lds + K_OFF + slot * TILE, qreg, 1, qi, hi);
      if ((k0 + BN - 1 > wv.all_hi) || (k0 < wv.all_lo)) {
        fp8_mask(sa, ln.all_hi, ln.all_lo, k0, hi);
        fp8_mask(sb, ln.all_hi, ln.all_lo, k0 + 32, hi);
      }
      fp8_softmax_tile<DB>(sa, sb, m_run, l_run, o_acc, pf, cs, thr);
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
  if (have_prev) fp8_pv<D>(o_acc, lds + I_OFF + ((n_tiles - 1) & 1) * TILE, pf, qi, hi);
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
  FA_LAUNCH(kern, dim3((unsigned)total), dim3(256), smem, stream, p, f8);
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
