// Forward attention on FP8 (OCP e4m3) q / k / v with per-(batch, kv head) descale factors; bf16 output, fp32 LSE.
//
// Contract (FA3's fp8 forward, hopper/flash_api.cpp): S = softmax_scale * q_descale * k_descale * (q . k^T) on the exact fp8
// values, P = softmax(S) rounded to e4m3 before the P.V product, out = P . (v_descale * v).
//
// Both products run on the block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 A and B, E8M0 scale 127 = 1.0 on both):
// twice the bf16 rate per clock (MI355X_MICROARCH.md, matrix cores).  The orientation is the project's: S^T = K.Q^T with
// the query on the lane (lane-local online softmax), O^T += V^T.P^T.
//
// Operand maps.  The kernel relies on one property of the instruction: lane l's operand byte j stands for the same k index
// in A and in B (probe_gfx950.hip checks it, with the A / B / D maps and the P^T pattern below, on exact integer data).  Then
//   - K and Q fragments are plain row reads: lane l takes 32 contiguous bytes of row l & 31 at head-dim offset 64 ks + 32 (l >> 5);
//   - P^T is the B operand straight from the two 32-key score accumulators of a 64-key tile, packed with v_cvt_pk_fp8_f32:
//     byte j of lane half h is key f(h, j) = 32 (j >> 4) + 8 ((j >> 2) & 3) + 4 h + (j & 3) of the tile (accumulator register j & 15);
//   - V^T, the A operand, must deliver V[f(h, j)][d] as byte j of lane (d, h).  Every tile is turned once into that image in LDS
//     (the transposed V image): 64 bytes per head-dim row d, lane (d, h) reads 32 contiguous bytes at 32 h.
//
// Numerics.  Scores are exact fp32 sums of exact fp8 products; c = softmax_scale * log2(e) * q_descale * k_descale is one
// fp32 constant, P = exp2(s c - m c).  The deferred rescale (FwdK::rescale_thr) is capped at 8 by the host so that P <= 256 < 448,
// the e4m3 maximum.  l sums the unrounded fp32 P; v_descale is folded into the epilogue's 1 / l.
//
// Schedule (4 waves, 128 query rows, Q fragments in registers, two workgroups per CU): iteration u DMAs K/V tile u+1,
// transposes V tile u into image u & 1, adds P_{u-1}.V_{u-1} from image (u-1) & 1, then scores tile u -- one barrier per tile.
// LDS: K0 | K1 | V0 | V1 | I0 | I1 (tile = 64 keys x D bytes; Q is staged in I0 | I1 before the loop).
#include <cstdio>

#include "fa_device.h"
#include "fa_kernel_params.h"
#include "fa_launch.h"

namespace fa {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// D = A.B + C on e4m3 A and B (cbsz = blgp = 0), unit E8M0 block scales (127 = 2^0) on both operands
FA_DEVINL f32x16 mfma_e4m3(i32x8 a, i32x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
}
FA_DEVINL i32x8 join16(u32x4 lo, u32x4 hi) {
  return __builtin_bit_cast(i32x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// 16-byte chunk swizzles.  Row tiles (K, V staging, Q): D = 128 -> 8 chunks per 128-byte row, D = 64 -> 4 per 64-byte row;
// chosen so that each 16-lane group of a ds_read_b128 (MI355X_MICROARCH.md §LDS: lanes {0-3, 12-15, 20-27}, ...) meets every
// 16-byte slot of a 256-byte bank row once.  V image rows are 64 bytes (4 chunks).
template <int D> FA_DEVINL constexpr int swz_row8(int row) {
  return D == 128 ? (((row >> 1) & 1) | (((row >> 3) & 1) << 1) | (((row >> 2) & 1) << 2)) : ((row >> 2) & 3);
}
FA_DEVINL constexpr int swz_img(int d) { return (d >> 2) & 3; }

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

  int b, h, m_block;
  if (p.work_list) {  // varlen: non-empty blocks only, heaviest first (fa_varlen_schedule_kernel)
    if (!work_list_item(p.work_list, blockIdx.x, p.h, p.h_k, b, h, m_block)) return;
  } else {
    const int w = xcd_interleave(blockIdx.x, p.n_units, p.unit_size, p.unit_hpx);
    if (w < 0) return;
    const int bh = w / p.nmb;
    const int mbr = w - bh * p.nmb;
    m_block = (p.wr >= 0) ? (p.nmb - 1 - mbr) : mbr;
    b = bh / p.h;
    h = bh - b * p.h;
  }
  const int hk = h / p.hk_ratio;

  int sq = p.sq, sk = p.sk;
  int64_t q_row0 = 0, k_row0 = 0;
  int64_t q_boff = (int64_t)b * p.q_bs, k_boff = (int64_t)b * p.k_bs, v_boff = (int64_t)b * p.v_bs, o_boff = (int64_t)b * p.o_bs;
  if (p.cu_q) { const int c0 = p.cu_q[b]; sq = p.cu_q[b + 1] - c0; q_row0 = c0; q_boff = 0; o_boff = 0; }
  if (p.cu_k) { const int c0 = p.cu_k[b]; sk = p.cu_k[b + 1] - c0; k_row0 = c0; k_boff = 0; v_boff = 0; }
  const int m0 = m_block * BM;
  if (m0 >= sq) return;

  const char* __restrict__ qp = (const char*)p.q + q_boff + q_row0 * p.q_rs + (int64_t)h * p.q_hs;
  const char* __restrict__ kp = (const char*)p.k + k_boff + k_row0 * p.k_rs + (int64_t)hk * p.k_hs;
  const char* __restrict__ vp = (const char*)p.v + v_boff + k_row0 * p.v_rs + (int64_t)hk * p.v_hs;
  __bf16* __restrict__ op = (__bf16*)p.o + o_boff + q_row0 * p.o_rs + (int64_t)h * p.o_hs;
  float* __restrict__ lsep = p.cu_q ? (p.lse + (int64_t)h * p.total_q + q_row0) : (p.lse + ((int64_t)b * p.h + h) * p.sq);

  const float qd = f8.q_descale ? f8.q_descale[(int64_t)b * f8.q_bs + (int64_t)hk * f8.q_hs] : 1.f;
  const float kd = f8.k_descale ? f8.k_descale[(int64_t)b * f8.k_bs + (int64_t)hk * f8.k_hs] : 1.f;
  const float vd = f8.v_descale ? f8.v_descale[(int64_t)b * f8.v_bs + (int64_t)hk * f8.v_hs] : 1.f;
  const float cs = p.scale_log2 * qd * kd;  // log2 units per unit of the raw fp8 dot product
  const float thr = p.rescale_thr;

  const int shift = sk - sq;
  const int blk_last = min(m0 + BM, sq) - 1;
  int kmax = sk - 1, kmin = 0;
  if (p.wr >= 0) kmax = min(kmax, blk_last + shift + p.wr);
  if (p.wl >= 0) kmin = max(0, m0 + shift - p.wl);
  const int n_min = kmin / BN;
  const int n_tiles = (kmax >= kmin) ? (kmax / BN + 1 - n_min) : 0;
  const int key_base = n_min * BN;

  const int w_row0 = m0 + wave * 32;
  const int w_row1 = min(w_row0 + 31, sq - 1);
  const bool wave_valid = w_row0 < sq;
  const int w_kmax = (p.wr >= 0) ? min(sk - 1, w_row1 + shift + p.wr) : sk - 1;
  const int w_kmin = (p.wl >= 0) ? max(0, w_row0 + shift - p.wl) : 0;
  const int w_full_hi = (p.wr >= 0) ? min(sk - 1, w_row0 + shift + p.wr) : sk - 1;
  const int w_full_lo = (p.wl >= 0) ? (w_row1 + shift - p.wl) : 0;
  const int my_row = w_row0 + qi;
  const bool row_valid = my_row < sq;
  const int lim_hi = (p.wr >= 0) ? min(sk - 1, my_row + shift + p.wr) : sk - 1;
  const int lim_lo = (p.wl >= 0) ? (my_row + shift - p.wl) : 0;

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
  {
    const int row = wave * 32 + qi;
    const char FA_LDS* rb = lds + I_OFF + row * ROW;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int c = 4 * ks + 2 * hi;
      qreg[ks] = join16(*(const u32x4 FA_LDS*)(rb + ((c ^ swz_row8<D>(row)) << 4)), *(const u32x4 FA_LDS*)(rb + (((c + 1) ^ swz_row8<D>(row)) << 4)));
    }
  }
  __syncthreads();  // the image buffers are written from the first iteration on

  // ---- V tile -> V^T image.  Thread (kg, dg) moves keys 4 kg .. 4 kg + 3 x head-dim columns 8 dg .. 8 dg + 7: four 8-byte row
  // reads, a 4 x 4 byte transpose per half (v_perm_b32), eight 4-byte writes at [d][pos(4 kg)].
  constexpr int T_UNITS = 16 * (D / 8);
  const int t_kg = tid & 15, t_dg = tid >> 4;
  const int t_key0 = 4 * t_kg;
  const int t_chunk = 2 * (t_kg & 1) + (t_kg >> 3);  // logical 16-byte chunk of the image row that holds these 4 keys
  const int t_inoff = 4 * ((t_kg >> 1) & 3);         // byte offset inside that chunk
  auto transpose_v = [&](int buf) __attribute__((always_inline)) {
    if (T_UNITS < NW * 64 && tid >= T_UNITS) return;
    const char FA_LDS* src = lds + V_OFF + buf * TILE;
    char FA_LDS* dst = lds + I_OFF + buf * TILE;
    u32x2 r[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int row = t_key0 + t;
      const int lc = t_dg >> 1;  // logical 16-byte chunk of the 8 columns
      r[t] = *(const u32x2 FA_LDS*)(src + row * ROW + ((lc ^ swz_row8<D>(row)) << 4) + (t_dg & 1) * 8);
    }
#pragma unroll
    for (int w = 0; w < 2; ++w) {  // columns 8 dg + 4 w .. + 3
      const unsigned a = r[0][w], bb = r[1][w], c = r[2][w], dd = r[3][w];
      // t0 = (a0 b0 a1 b1), t1 = (a2 b2 a3 b3), t2 = (c0 d0 c1 d1), t3 = (c2 d2 c3 d3)  [bytes listed low to high]
      const unsigned t0 = __builtin_amdgcn_perm(bb, a, 0x05010400u);
      const unsigned t1 = __builtin_amdgcn_perm(bb, a, 0x07030602u);
      const unsigned t2 = __builtin_amdgcn_perm(dd, c, 0x05010400u);
      const unsigned t3 = __builtin_amdgcn_perm(dd, c, 0x07030602u);
      const unsigned o[4] = {__builtin_amdgcn_perm(t2, t0, 0x05040100u), __builtin_amdgcn_perm(t2, t0, 0x07060302u),
                             __builtin_amdgcn_perm(t3, t1, 0x05040100u), __builtin_amdgcn_perm(t3, t1, 0x07060302u)};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int d = 8 * t_dg + 4 * w + e;
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

  // O^T += V^T.P^T from image `buf`: row d = 32 db + qi, logical chunks 2 hi (keys of score accumulator A) and 2 hi + 1 (B)
  auto pv = [&](int buf) __attribute__((always_inline)) {
    const char FA_LDS* img = lds + I_OFF + buf * TILE;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const int d = 32 * db + qi;
      const char FA_LDS* rb = img + d * 64;
      const i32x8 vt = join16(*(const u32x4 FA_LDS*)(rb + (((2 * hi) ^ swz_img(d)) << 4)), *(const u32x4 FA_LDS*)(rb + (((2 * hi + 1) ^ swz_img(d)) << 4)));
      o_acc[db] = mfma_e4m3(vt, pf, o_acc[db]);
    }
  };
  // S^T of one 32-key half of K tile `buf`
  auto qk_half = [&](f32x16& s, int buf, int half) __attribute__((always_inline)) {
    const int row = 32 * half + qi;
    const char FA_LDS* rb = lds + K_OFF + buf * TILE + row * ROW;
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
  // registers 4g .. 4g+3 -> bytes 0 .. 3 of dword base + g (word_sel 0: bytes 0, 1; word_sel 1: bytes 2, 3)
  auto pack = [&](const f32x16& s, int base) __attribute__((always_inline)) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      int w = __builtin_amdgcn_cvt_pk_fp8_f32(s[4 * g], s[4 * g + 1], 0, false);
      w = __builtin_amdgcn_cvt_pk_fp8_f32(s[4 * g + 2], s[4 * g + 3], w, true);
      pf[base + g] = w;
    }
  };

  for (int u = 0; u < n_tiles; ++u) {
    const int buf = u & 1;
    if (u + 1 < n_tiles) { dma_tile(false, buf ^ 1, u + 1); dma_tile(true, buf ^ 1, u + 1); }
    transpose_v(buf);
    if (have_prev) pv(buf ^ 1);
    const int k0 = key_base + u * BN;
    const bool active = wave_valid && k0 <= w_kmax && k0 + BN - 1 >= w_kmin;
    if (active) {
      f32x16 sa, sb;
      qk_half(sa, buf, 0);
      qk_half(sb, buf, 1);
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
    lds_dma_wait_all();  // this wave's DMA pieces have landed ...
    __syncthreads();     // ... and everybody's pieces and image rows are visible
  }
  if (have_prev) pv((n_tiles - 1) & 1);
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
  hipLaunchKernelGGL(kern, dim3((unsigned)total), dim3(256), smem, stream, p, f8);
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
