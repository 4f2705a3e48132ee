// Forward attention on FP8 (OCP e4m3) q / k / v with per-(batch, kv head) descale factors; bf16 output, fp32 LSE.
//
// Contract, operand maps, the transposed V image and the numerics: fa_fp8_tile.h, which holds the tile code this kernel shares with the
// KV-cache kernel (fa_fwd_fp8_kv.hip).  Block geometry and masks: fa_fwd_block.h.  This file owns the schedule, varlen and the work list.
//
// Schedule (4 waves, 128 query rows, Q fragments in registers, two workgroups per CU): iteration u DMAs K/V tile u+1,
// transposes V tile u into image u & 1, adds P_{u-1}.V_{u-1} from image (u-1) & 1, then scores tile u -- one barrier per tile.
// LDS: K0 | K1 | V0 | V1 | I0 | I1 (tile = 64 keys x D bytes; Q is staged in I0 | I1 before the loop).
#include <cstdio>

#include "fa_device.h"
#include "fa_fp8_tile.h"
#include "fa_fwd_block.h"
#include "fa_kernel_params.h"
#include "fa_launch.h"

namespace fa {

template <int D>
__global__ void __launch_bounds__(256, 2) fa_fwd_fp8_kernel(const FwdK p, const Fp8K f8) {
  constexpr int NW = 4, BM = NW * 32, BN = 64;
  constexpr int ROW = D;                  // bytes per K / V / Q row
  constexpr int TILE = BN * ROW;          // bytes per K / V tile and per V image
  constexpr int CPR = D / 16;             // 16-byte chunks per row
  constexpr int KS = D / 64;              // MFMAs per 32-key half tile of S^T
  constexpr int DB = D / 32;              // 32-row blocks of O^T
  constexpr int K_OFF = 0, V_OFF = 2 * TILE, I_OFF = 4 * TILE;
  static_assert(D == 64 || D == 128, "head dims built: 64, 128");
  constexpr float kLn2 = 0.6931471805599453f;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char FA_LDS* lds = (char FA_LDS*)smem;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, qi = lane & 31;

  constexpr int F = FB_LIST | FB_VARLEN;  // the host contract: no packing, key splits, cache arguments, seqused_* or leftpad_k
  FwdWork wk;
  if (!fwd_work<F>(p, blockIdx.x, wk)) return;
  const int b = wk.b, h = wk.h, hk = h / p.hk_ratio;
  const FwdSeq seq = fwd_seq<F>(p, b);
  const int sq = seq.sq, sk = seq.sk;
  const int m0 = wk.m_block * BM;
  if (m0 >= sq) return;

  const char* __restrict__ qp = (const char*)p.q + seq.q_off + (int64_t)h * p.q_hs;
  const char* __restrict__ kp = (const char*)p.k + seq.k_off + (int64_t)hk * p.k_hs;
  const char* __restrict__ vp = (const char*)p.v + seq.v_off + (int64_t)hk * p.v_hs;
  __bf16* __restrict__ op = (__bf16*)p.o + seq.o_off + (int64_t)h * p.o_hs;
  float* __restrict__ lsep = fwd_lse_row<F>(p, seq, b, h);

  const float qd = f8.q_descale ? f8.q_descale[(int64_t)b * f8.q_bs + (int64_t)hk * f8.q_hs] : 1.f;
  const float kd = f8.k_descale ? f8.k_descale[(int64_t)b * f8.k_bs + (int64_t)hk * f8.k_hs] : 1.f;
  const float vd = f8.v_descale ? f8.v_descale[(int64_t)b * f8.v_bs + (int64_t)hk * f8.v_hs] : 1.f;
  const float cs = p.scale_log2 * qd * kd;  // log2 units per unit of the raw fp8 dot product
  const float thr = p.rescale_thr;

  // ---- key tiles of the block, visibility limits of this wave's 32 rows and of this lane's row ----
  const int shift = sk - sq;  // bottom-right alignment
  const TileRange tr = tile_range<F>(p, key_window(m0, min(m0 + BM, sq) - 1, shift, sk, p.wl, p.wr), 0);
  const int n_min = tr.n_min, n_tiles = tr.n_tiles, key_base = n_min * BN;
  const int w_row0 = m0 + wave * 32, my_row = w_row0 + qi;
  const bool wave_valid = w_row0 < sq, row_valid = my_row < sq;
  const KeyWindow wv = key_window(w_row0, min(w_row0 + 31, sq - 1), shift, sk, p.wl, p.wr);
  const KeyWindow ln = key_window(my_row, my_row, shift, sk, p.wl, p.wr);

  // ---- K / V tiles global -> LDS by DMA (1 KiB per wave instruction, lane-linear destination; the swizzle is applied to the
  // per-lane source chunk).  Rows past the last key are clamped to the last key: finite data, their scores are masked.
  constexpr int RPD = 1024 / ROW;        // tile rows per DMA instruction
  constexpr int DPW = TILE / 1024 / NW;  // DMA instructions per wave and tile
  static_assert(DPW >= 1 && (TILE / 1024) % NW == 0, "tile does not divide over the waves");
  const int d_row = lane / CPR, d_pc = lane % CPR;
  auto dma_tile = [&](bool is_v, int buf, int t) __attribute__((always_inline)) {
    const int n = n_min + t;
    const int64_t rs = is_v ? p.v_rs : p.k_rs;
    const char* base = (is_v ? vp : kp) + (int64_t)n * BN * rs;
    char FA_LDS* dst = lds + (is_v ? V_OFF : K_OFF) + buf * TILE + wave * DPW * 1024;
#pragma unroll
    for (int i = 0; i < DPW; ++i) {
      const int row = (wave * DPW + i) * RPD + d_row;
      const int grow = min(n * BN + row, sk - 1) - n * BN;
      lds_dma_16B(base + (int64_t)grow * rs + ((d_pc ^ swz_row8<D>(row)) << 4), dst + i * 1024);
    }
  };

  // Q block -> LDS (the two image buffers, unused until the loop) -> registers
  {
    constexpr int QDMA = BM * ROW / 1024 / NW;
#pragma unroll
    for (int i = 0; i < QDMA; ++i) {
      const int row = (wave * QDMA + i) * RPD + d_row;
      const int grow = min(m0 + row, sq - 1);
      lds_dma_16B(qp + (int64_t)grow * p.q_rs + ((d_pc ^ swz_row8<D>(row)) << 4), lds + I_OFF + (wave * QDMA + i) * 1024);
    }
  }
  if (n_tiles > 0) { dma_tile(false, 0, 0); dma_tile(true, 0, 0); }
  lds_dma_wait_all();
  __syncthreads();
  i32x8 qreg[KS];
  fp8_read_q<D>(qreg, lds + I_OFF, wave * 32 + qi, hi);
  __syncthreads();  // the image buffers are written from the first iteration on

  f32x16 o_acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[db][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  i32x8 pf = {0, 0, 0, 0, 0, 0, 0, 0};  // packed P^T of the previous tile (B operand)
  bool have_prev = false;

  for (int u = 0; u < n_tiles; ++u) {
    const int buf = u & 1;
    if (u + 1 < n_tiles) { dma_tile(false, buf ^ 1, u + 1); dma_tile(true, buf ^ 1, u + 1); }
    fp8_transpose_v<D, NW * 64>(lds + V_OFF + buf * TILE, lds + I_OFF + buf * TILE, tid);
    if (have_prev) fp8_pv<D>(o_acc, lds + I_OFF + (buf ^ 1) * TILE, pf, qi, hi);
    const int k0 = key_base + u * BN;
    const bool active = wave_valid && k0 <= wv.any_hi && k0 + BN - 1 >= wv.any_lo;
    if (active) {
      f32x16 sa, sb;
      fp8_qk_half<D>(sa, lds + K_OFF + buf * TILE, qreg, 0, qi, hi);
      fp8_qk_half<D>(sb, lds + K_OFF + buf * TILE, qreg, 1, qi, hi);
      if ((k0 + BN - 1 > wv.all_hi) || (k0 < wv.all_lo)) {
        fp8_mask(sa, ln.all_hi, ln.all_lo, k0, hi);
        fp8_mask(sb, ln.all_hi, ln.all_lo, k0 + 32, hi);
      }
      fp8_softmax_tile<DB>(sa, sb, m_run, l_run, o_acc, pf, cs, thr);
    }
    have_prev = active;
    lds_dma_wait_all();  // this wave's DMA pieces have landed ...
    __syncthreads();     // ... and everybody's pieces and image rows are visible
  }
  if (have_prev) fp8_pv<D>(o_acc, lds + I_OFF + ((n_tiles - 1) & 1) * TILE, pf, qi, hi);
  __syncthreads();  // every wave is done with the images before the epilogue stages O over them

  if (!wave_valid) return;
  const float l_tot = half_sum(l_run);
  const bool dead = (l_tot == 0.f) || (l_tot != l_tot);
  const float inv = dead ? 1.f : vd / l_tot;
  store_tile_via_lds<__bf16, D>(lds + wave * 32 * (2 * D + 16), o_acc, inv, op + (int64_t)w_row0 * p.o_rs, p.o_rs, sq - w_row0, lane);
  if (row_valid && hi == 0) lsep[my_row] = dead ? INFINITY : (m_run * cs * kLn2 + __logf(l_tot));
}

template <int D>
static int launch_fwd_fp8_t(const FwdK& p, const Fp8K& f8, hipStream_t stream) {
  constexpr int smem = 6 * 64 * D;
  static_assert(4 * 32 * (2 * D + 16) <= smem, "epilogue staging does not fit");
  auto kern = fa_fwd_fp8_kernel<D>;
  static std::atomic<unsigned long long> attr_mask{0};  // LDS is addressed by byte offset: the dynamic segment must start at 0
  if (ensure_dyn_lds(attr_mask, (const void*)kern, smem, true) != 0) return -1;
  const long long total = p.work_list ? (long long)p.work_bound * p.h : units_grid(p.n_units, p.unit_size);
  if (total <= 0) return 0;
  FA_LAUNCH(kern, dim3((unsigned)total), dim3(256), smem, stream, p, f8);
  if (hipGetLastError() != hipSuccess) return -1;
  LastSchedule& ls = last_schedule();
  ls.fwd_kernel = 4; ls.fwd_nw = 4; ls.fwd_feat = 0; ls.fwd_splits = 1; ls.fwd_list = p.work_list != nullptr; ls.d = D;
  ls.bf16 = 0; ls.fwd_pack = 1;
  snprintf(ls.name, sizeof(ls.name), "fa::fa_fwd_fp8_kernel<e4m3,%d,4>", D);
  return 0;
}

int launch_fwd_fp8(const FwdK& p, const Fp8K& f8, int d, hipStream_t stream) {
  if ((uint64_t)64 * (uint64_t)(p.k_rs > p.v_rs ? p.k_rs : p.v_rs) >= (1ull << 31)) return -3;
  if (d == 128) return launch_fwd_fp8_t<128>(p, f8, stream);
  if (d == 64) return launch_fwd_fp8_t<64>(p, f8, stream);
  return -2;
}

}  // namespace fa
