// Fused attention forward for a value head dim that differs from the query / key head dim (DeepSeek-V2/V3 style multi-head latent
// attention: 192 Q/K channels -- 128 "nope" + 64 rotary -- and 128 V channels per head), gfx950 (MI355X).
//
// The reference's newer interface takes this shape as given ("Q/K headdim in (128, 192] and V headdim in (96, 128]",
// hopper/flash_api.cpp:782-786).  The structure is the lock-step schedule of fa_fwd_kernel (fa_fwd.hip: S^T = K.Q^T on
// v_mfma_f32_32x32x16, lane-local online softmax, O^T += V^T.P^T with the key permutation applied to the transpose reads of V,
// LDS-DMA tile feed, the same (batch, head, query block) decode, masks and "no visible key => out = 0, lse = +inf" rule), with ONE
// difference that the 256-pitch kernel serving head dim 192 cannot have: K and V tiles have their own row pitch.
//
//   K tile  64 keys x 192 channels = 24 KB  (pitch 384 B),   S^T runs DQK / 16 = 12 k-steps
//   V tile  64 keys x 128 channels = 16 KB  (pitch 256 B),   O^T has DV / 32 = 4 output blocks
//
// Double-buffered that is 80 KB per workgroup -- half of the CU's 160 KiB, so two 4-wave workgroups share a CU (two waves per
// SIMD: one wave's softmax runs under the other's MFMAs) where the 256-pitch kernel (128 KB) runs one.  The Q block (128 x 384 B =
// 48 KB) is staged through the same space before the first tile and the O tile (128 x 272 B) after the last one.
//
// Swizzles.  A bank row of the LDS is 256 B = sixteen 16-byte slots (ds_read_b128 and ds_read_b64_tr_b16 both bank on (addr / 4) % 64).
//   K, pitch 384 B = 256 + 128: row r starts at slot 8 * (r & 1) of its bank row, exactly as a 128-byte pitch does, so the 16 lanes
//     of a ds_read_b128 group (8 even + 8 odd rows: {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31}), all asking for chunk c, land on two
//     8-slot halves; XOR-ing the chunk's low three bits with (r >> 1) & 7 -- the pitch-64 rule of fa_fwd.hip -- gives the 8 rows of
//     one parity 8 different slots ((r >> 1) & 7 takes every value once per parity in either group), the XOR never leaves the
//     8-chunk group, so chunk c < 24 stays inside the row, and row r + 32 (the second key block: + 3 * 256 * 16 B) banks like row r.
//   V, pitch 256 B: one row = one bank row.  A half-wave's transpose read covers rows 4 * hi + (0..3) (+ 8 / 16 * k), 64 B of each;
//     XOR-ing the 64-byte quarter index with row & 3 puts the four rows on four different quarters, and inside a quarter the
//     (lane >> 4) & 1 half and the four 8-byte columns are distinct: 32 lanes x 8 B = all 64 banks once (fa_fwd.hip's pitch-128 rule).
#include <cstdio>
#include <type_traits>

#include "fa_device.h"
#include "fa_fwd_block.h"
#include "fa_kernel_params.h"
#include "fa_launch.h"

namespace fa {

FA_DEVINL constexpr int kdv_swz(int row) { return (row >> 1) & 7; }   // K / Q rows, 16-byte chunks (pitch 384 B)
FA_DEVINL constexpr int vdv_swz(int row) { return row & 3; }          // V rows, 64-byte quarters (pitch 256 B)

template <int N> using ICdv = std::integral_constant<int, N>;

template <typename E, int DQK, int DV, int NW>
__global__ void __launch_bounds__(NW * 64, 2) fa_fwd_dv_kernel(const FwdK p) {
  using T = ElemTraits<E>;
  using V8 = typename T::v8;
  constexpr int BM = NW * 32, BN = 64;
  constexpr int KCPR = DQK / 8, VCPR = DV / 8;          // 16-byte chunks per K / V row
  constexpr int KROW = DQK * 2, VROW = DV * 2;          // row pitches in bytes
  constexpr int KT = BN * KROW, VT = BN * VROW;         // tile bytes
  constexpr int KS = DQK / 16, DB = DV / 32;
  constexpr int OFF_K = 0, OFF_V = 2 * KT;              // K0 | K1 | V0 | V1
  static_assert(DQK == 192 && DV == 128, "swizzles and pitches are derived for (192, 128)");
  static_assert(KT % (1024 * NW) == 0 && VT % (1024 * NW) == 0 && (32 * KROW) % 1024 == 0, "tiles do not divide over the waves");
  static_assert(2 * KT + 2 * VT <= 80 * 1024 && BM * KROW <= 2 * KT + 2 * VT && BM * (VROW + 16) <= 2 * KT + 2 * VT, "80 KB: two workgroups per CU");
  constexpr float kLn2 = 0.6931471805599453f;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char FA_LDS* lds = (char FA_LDS*)smem;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, qi = lane & 31;

  // ---- which (batch, head, query block), its sequence, key tiles and visibility limits: fa_fwd_block.h ----
  constexpr int F = FB_LIST | FB_VARLEN | FB_SEQUSED;  // the host contract: no packing, key splits, cache arguments or leftpad_k
  FwdWork wk;
  if (!fwd_work<F>(p, blockIdx.x, wk)) return;
  const int b = wk.b, h = wk.h, hk = h / p.hk_ratio;
  const FwdSeq seq = fwd_seq<F>(p, b);
  const int sq = seq.sq, sk = seq.sk;
  const int m0 = wk.m_block * BM;
  if (m0 >= sq) return;

  const E* __restrict__ qp = (const E*)p.q + seq.q_off + (int64_t)h * p.q_hs;
  const E* __restrict__ kp = (const E*)p.k + seq.k_off + (int64_t)hk * p.k_hs;
  const E* __restrict__ vp = (const E*)p.v + seq.v_off + (int64_t)hk * p.v_hs;
  E* __restrict__ op = (E*)p.o + seq.o_off + (int64_t)h * p.o_hs;
  float* __restrict__ lsep = fwd_lse_row<F>(p, seq, b, h);

  const int shift = sk - sq;  // bottom-right alignment
  const TileRange tr = tile_range<F>(p, key_window(m0, min(m0 + BM, sq) - 1, shift, sk, p.wl, p.wr), 0);
  const int n_min = tr.n_min, n_tiles = tr.n_tiles;
  const int w_row0 = m0 + wave * 32, my_row = w_row0 + qi;
  const bool wave_valid = w_row0 < sq, row_valid = my_row < sq;
  const KeyWindow wv = key_window(w_row0, min(w_row0 + 31, sq - 1), shift, sk, p.wl, p.wr);  // this wave's 32 rows
  const KeyWindow ln = key_window(my_row, my_row, shift, sk, p.wl, p.wr);                      // this lane's row
  const float cs = p.scale_log2;
  const float thr = p.rescale_thr;

  // ---- LDS-DMA staging: 1 KiB per wave instruction, lane-linear destination, so piece pi of a tile holds the 16-byte positions
  // 64 * pi + lane; position L is (row L / CPR, chunk position L % CPR) and fetches the SOURCE chunk the swizzle assigns to it.  A
  // 384-byte K row is 24 positions: a piece covers 2 2/3 rows, whence the division.  Rows past the last key are clamped to it. ----
  constexpr int KDPW = KT / 1024 / NW, VDPW = VT / 1024 / NW;
  auto dma_k = [&](int buf, int n) __attribute__((always_inline)) {
    const E* base = kp + (int64_t)n * BN * p.k_rs;
    char FA_LDS* dst = lds + OFF_K + buf * KT + wave * KDPW * 1024;
#pragma unroll
    for (int i = 0; i < KDPW; ++i) {
      const int L = (wave * KDPW + i) * 64 + lane;
      const int row = L / KCPR, pc = L - row * KCPR;
      const int grow = min(n * BN + row, sk - 1) - n * BN;
      const int c = pc ^ kdv_swz(row);
      lds_dma_16B(base + (int64_t)grow * p.k_rs + c * 8, dst + i * 1024);
    }
  };
  auto dma_v = [&](int buf, int n) __attribute__((always_inline)) {
    const E* base = vp + (int64_t)n * BN * p.v_rs;
    char FA_LDS* dst = lds + OFF_V + buf * VT + wave * VDPW * 1024;
#pragma unroll
    for (int i = 0; i < VDPW; ++i) {
      const int row = (wave * VDPW + i) * (64 / VCPR) + lane / VCPR, pc = lane % VCPR;
      const int grow = min(n * BN + row, sk - 1) - n * BN;
      const int c = (((pc >> 2) ^ vdv_swz(row)) << 2) | (pc & 3);
      lds_dma_16B(base + (int64_t)grow * p.v_rs + c * 8, dst + i * 1024);
    }
  };

  // ---- Q fragments (B operand of S^T = K.Q^T): lane = query row, 8 consecutive channels per k-step ----
  V8 qf[KS];
  if (sq >= 64) {  // each wave DMAs its own 32 rows into the idle LDS (K-style swizzle) and copies its fragments to registers
    constexpr int QDPW = 32 * KROW / 1024;
    char FA_LDS* qdst = lds + wave * 32 * KROW;
#pragma unroll
    for (int i = 0; i < QDPW; ++i) {
      const int L = i * 64 + lane;
      const int row = L / KCPR, pc = L - row * KCPR;
      const int grow = min(m0 + wave * 32 + row, sq - 1);
      const int c = pc ^ kdv_swz(row);
      lds_dma_16B(qp + (int64_t)grow * p.q_rs + c * 8, qdst + i * 1024);
    }
    lds_dma_wait_all();
    const char FA_LDS* qb = qdst + qi * KROW;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = bitcast_u32x4<V8>(*(const u32x4 FA_LDS*)(qb + (((2 * ks + hi) ^ kdv_swz(qi)) << 4)));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();  // the K/V tile DMA below reuses this LDS
  } else {           // few query rows (decode): 16-byte loads at row stride
    const E* qrow = qp + (int64_t)my_row * p.q_rs + 8 * hi;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = bitcast_u32x4<V8>(ld_global_16B(qrow + 16 * ks, row_valid));
  }

  // ---- per-lane LDS read addresses (loop invariant; buffers, k-steps past the swizzled 8-chunk group and sub-tiles are immediates) ----
  int kaddr[4];   // k-step ks reads chunk 2 ks + hi = 8 * (ks >> 2) + (2 * (ks & 3) + hi): only the low three bits are swizzled
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) kaddr[k4] = qi * KROW + (((2 * k4 + hi) ^ kdv_swz(qi)) << 4);
  const int tr_i = lane & 15, tr_half = (lane >> 4) & 1;
  const int tr_rr = tr_i >> 2, tr_cc = tr_i & 3;
  int vaddr[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) vaddr[db] = (4 * hi + tr_rr) * VROW + ((db ^ vdv_swz(tr_rr)) << 6) + tr_half * 32 + tr_cc * 8;

  // ---- online-softmax state (per lane = per query row; both half-waves keep identical m) ----------
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
    return wave_valid && (j < n_tiles) && (kv0 <= wv.any_hi) && (kv0 + BN - 1 >= wv.any_lo);
  };

  // S^T[key][query] of the tile in K buffer `buf`: 12 k-steps x 2 key blocks; operand reads run PF k-steps ahead of their MFMAs
  auto qk = [&](auto bufc) __attribute__((always_inline)) {
    constexpr int buf = decltype(bufc)::value;
    const char FA_LDS* kbuf = lds + OFF_K + buf * KT;
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

  // mask + online softmax of s -> pf (P^T as B operand), updates m_run / l_run / o_acc scale (fa_fwd_kernel's rule, plain variant)
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

  // O^T[d][query] += V^T[d][key] . P^T[key][query]: 4 key groups x 4 output blocks; transpose reads run PFV MFMAs ahead
  auto pv = [&](auto bufc) __attribute__((always_inline)) {
    constexpr int buf = decltype(bufc)::value;
    const char FA_LDS* vbuf = lds + OFF_V + buf * VT;
    constexpr int NOP = 4 * DB, PFV = 4;
    s16x4 vlo[PFV], vhi[PFV];
#pragma unroll
    for (int i = 0; i < PFV - 1; ++i) {
      vlo[i % PFV] = lds_read_tr16(vbuf + vaddr[i % DB] + (16 * (i / DB)) * VROW);
      vhi[i % PFV] = lds_read_tr16(vbuf + vaddr[i % DB] + (16 * (i / DB) + 8) * VROW);
    }
#pragma unroll
    for (int i = 0; i < NOP; ++i) {
      const int nx = i + PFV - 1;
      if (nx < NOP) {
        vlo[nx % PFV] = lds_read_tr16(vbuf + vaddr[nx % DB] + (16 * (nx / DB)) * VROW);
        vhi[nx % PFV] = lds_read_tr16(vbuf + vaddr[nx % DB] + (16 * (nx / DB) + 8) * VROW);
      }
      __builtin_amdgcn_sched_barrier(0);
      o_acc[i % DB] = T::mfma(combine_tr<V8>(vlo[i % PFV], vhi[i % PFV]), pf[i / DB], o_acc[i % DB]);
    }
  };

  // ---- lock-step key loop: per tile {DMA the next tile into the other buffers, QK^T, softmax, PV, wait, barrier} ----
  if (n_tiles > 0) {
    dma_k(0, n_min);
    dma_v(0, n_min);
    lds_dma_wait_all();
    __syncthreads();
  }
  auto step = [&](auto bufc, int j) __attribute__((always_inline)) {
    constexpr int buf = decltype(bufc)::value;
    if (j + 1 < n_tiles) {  // lands in the other buffers while this tile is being computed
      dma_k(buf ^ 1, n_min + j + 1);
      dma_v(buf ^ 1, n_min + j + 1);
    }
    if (tile_active(j)) {
      qk(bufc);
      softmax_step(j);
      pv(bufc);
    }
    lds_dma_wait_all();  // this wave's pieces have landed ...
    __syncthreads();     // ... and everybody's are visible before the next tile reads them
  };
  for (int j = 0; j < n_tiles; j += 2) {
    step(ICdv<0>{}, j);
    if (j + 1 < n_tiles) step(ICdv<1>{}, j + 1);
  }

  // ---- epilogue: normalise, store O through the freed tile space (whole-row stores) and LSE ----
  if (!wave_valid) return;
  const float l_tot = half_sum(l_run);
  const bool dead = (l_tot == 0.f) || (l_tot != l_tot);  // no visible key: out = 0, lse = +inf
  const float inv = dead ? 1.f : 1.f / l_tot;
  store_tile_via_lds<E, DV, DV>(lds + wave * 32 * (VROW + 16), o_acc, inv, op + (int64_t)w_row0 * p.o_rs, p.o_rs, sq - w_row0, lane);
  if (row_valid && hi == 0) lsep[my_row] = dead ? INFINITY : (m_run * cs * kLn2 + __logf(l_tot));
}

template <typename E>
static int launch_fwd_dv_e(const FwdK& p, hipStream_t stream) {
  constexpr int NW = 4, DQK = 192, DV = 128;
  constexpr int smem = 2 * 64 * DQK * 2 + 2 * 64 * DV * 2;   // 80 KB: K / V double buffers; the Q prologue and the O epilogue reuse them
  auto kern = fa_fwd_dv_kernel<E, DQK, DV, NW>;
  static std::atomic<unsigned long long> attr_mask{0};
  if (ensure_dyn_lds(attr_mask, (const void*)kern, smem) != 0) return -1;
  const long long total = p.work_list ? (long long)p.work_bound * p.h : units_grid(p.n_units, p.unit_size);  // (the list names every non-empty block)
  if (total <= 0) return 0;
  FA_LAUNCH(kern, dim3((unsigned)total), dim3(NW * 64), smem, stream, p);
  if (hipGetLastError() != hipSuccess) return -1;
  LastSchedule& ls = last_schedule();
  ls.fwd_kernel = 6; ls.fwd_nw = NW; ls.fwd_feat = FEAT_NONE; ls.fwd_splits = 1; ls.fwd_list = p.work_list != nullptr; ls.d = DQK; ls.dv = DV;
  ls.bf16 = std::is_same<E, __bf16>::value;
  snprintf(ls.name, sizeof(ls.name), "fa::fa_fwd_dv_kernel<%s,%d,%d,%d>", ls.bf16 ? "bf16" : "f16", DQK, DV, NW);
  return 0;
}

int launch_fwd_dv(const FwdK& p, int dtype_bf16, int d, int dv, hipStream_t stream) {
  if (d != 192 || dv != 128) return -2;
  // a tile is addressed from its first row with 64-bit per-lane addresses; nothing to bound beyond the contract's strides
  return dtype_bf16 ? launch_fwd_dv_e<__bf16>(p, stream) : launch_fwd_dv_e<_Float16>(p, stream);
}

}  // namespace fa
