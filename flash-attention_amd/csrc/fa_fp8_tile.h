// The e4m3 tile code of the FP8 forward kernels (fa_fwd_fp8.hip, fa_fwd_fp8_kv.hip): operand reads, the transposed V image, the two
// products, the mask and the online-softmax step of one 64-key tile.  The kernels own their schedules; this header owns the maths.
//
// Contract (FA3's fp8 forward, hopper/flash_api.cpp): S = softmax_scale * q_descale * k_descale * (q . k^T) on the exact fp8
// values, P = softmax(S) rounded to e4m3 before the P.V product, out = P . (v_descale * v).
//
// Both products run on the block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 A and B, E8M0 scale 127 = 1.0 on both):
// twice the bf16 rate per clock (MI355X_MICROARCH.md, matrix cores).  The orientation is the project's: S^T = K.Q^T with
// the query on the lane (lane-local online softmax), O^T += V^T.P^T.
//
// Operand maps.  The kernels rely on one property of the instruction: lane l's operand byte j stands for the same k index
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
// Throughout: D = head dim = bytes per K / V / Q row, a tile is 64 keys x D bytes, qi = lane & 31, hi = lane >> 5.
#pragma once
#include "fa_device.h"

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

// the 32 bytes lane half `hi` takes of k-step `ks` of the swizzled row at `rb` (a K, or a staged Q, row)
template <int D> FA_DEVINL i32x8 fp8_row_frag(const char FA_LDS* rb, int row, int ks, int hi) {
  const int c = 4 * ks + 2 * hi;
  return join16(*(const u32x4 FA_LDS*)(rb + ((c ^ swz_row8<D>(row)) << 4)), *(const u32x4 FA_LDS*)(rb + (((c + 1) ^ swz_row8<D>(row)) << 4)));
}

// Q fragments (B operand of S^T) of row `row` of the Q block staged at `qblock` with the row-tile swizzle
template <int D> FA_DEVINL void fp8_read_q(i32x8 (&qreg)[D / 64], const char FA_LDS* qblock, int row, int hi) {
  const char FA_LDS* rb = qblock + row * D;
#pragma unroll
  for (int ks = 0; ks < D / 64; ++ks) qreg[ks] = fp8_row_frag<D>(rb, row, ks, hi);
}

// V tile `src` -> V^T image `dst`.  Thread (kg, dg) = (tid & 15, tid >> 4) moves keys 4 kg .. 4 kg + 3 x head-dim columns 8 dg .. 8 dg + 7:
// four 8-byte row reads, a 4 x 4 byte transpose per half (v_perm_b32), eight 4-byte writes at [d][pos(4 kg)].  NT = threads of the workgroup.
template <int D, int NT> FA_DEVINL void fp8_transpose_v(const char FA_LDS* src, char FA_LDS* dst, int tid) {
  constexpr int T_UNITS = 16 * (D / 8);
  if (T_UNITS < NT && tid >= T_UNITS) return;
  const int t_kg = tid & 15, t_dg = tid >> 4;
  const int t_key0 = 4 * t_kg;
  const int t_chunk = 2 * (t_kg & 1) + (t_kg >> 3);  // logical 16-byte chunk of the image row that holds these 4 keys
  const int t_inoff = 4 * ((t_kg >> 1) & 3);         // byte offset inside that chunk
  u32x2 r[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = t_key0 + t;
    const int lc = t_dg >> 1;  // logical 16-byte chunk of the 8 columns
    r[t] = *(const u32x2 FA_LDS*)(src + row * D + ((lc ^ swz_row8<D>(row)) << 4) + (t_dg & 1) * 8);
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
}

// O^T += V^T.P^T from image `img`: row d = 32 db + qi, logical chunks 2 hi (keys of score accumulator A) and 2 hi + 1 (B)
template <int D> FA_DEVINL void fp8_pv(f32x16 (&o_acc)[D / 32], const char FA_LDS* img, i32x8 pf, int qi, int hi) {
#pragma unroll
  for (int db = 0; db < D / 32; ++db) {
    const int d = 32 * db + qi;
    const char FA_LDS* rb = img + d * 64;
    const i32x8 vt = join16(*(const u32x4 FA_LDS*)(rb + (((2 * hi) ^ swz_img(d)) << 4)), *(const u32x4 FA_LDS*)(rb + (((2 * hi + 1) ^ swz_img(d)) << 4)));
    o_acc[db] = mfma_e4m3(vt, pf, o_acc[db]);
  }
}

// S^T of one 32-key half of the K tile at `ktile`
template <int D> FA_DEVINL void fp8_qk_half(f32x16& s, const char FA_LDS* ktile, const i32x8 (&qreg)[D / 64], int half, int qi, int hi) {
  const int row = 32 * half + qi;
  const char FA_LDS* rb = ktile + row * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < D / 64; ++ks) s = mfma_e4m3(fp8_row_frag<D>(rb, row, ks, hi), qreg[ks], s);
}

// keys outside [lim_lo, lim_hi] of this lane's query -> -inf; k0 = first key of the 32-key accumulator
FA_DEVINL void fp8_mask(f32x16& s, int lim_hi, int lim_lo, int k0, int hi) {
  const int rel_hi = lim_hi - k0 - 4 * hi;
  const int rel_lo = lim_lo - k0 - 4 * hi;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int off = acc_row(r, 0);
    s[r] = ((off <= rel_hi) && (off >= rel_lo)) ? s[r] : -INFINITY;
  }
}

// registers 4g .. 4g+3 -> bytes 0 .. 3 of dword base + g (word_sel 0: bytes 0, 1; word_sel 1: bytes 2, 3)
FA_DEVINL void fp8_pack(i32x8& pf, const f32x16& s, int base) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(s[4 * g], s[4 * g + 1], 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(s[4 * g + 2], s[4 * g + 3], w, true);
    pf[base + g] = w;
  }
}

// Online softmax of one 64-key tile: the (masked) raw scores sa | sb become P, rounded to e4m3 into pf (the B operand of the tile's
// P.V product); m_run / l_run follow, o_acc is rescaled when some row's maximum grew by more than thr (log2 units).
template <int DB> FA_DEVINL void fp8_softmax_tile(f32x16& sa, f32x16& sb, float& m_run, float& l_run, f32x16 (&o_acc)[DB], i32x8& pf, float cs, float thr) {
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
  fp8_pack(pf, sa, 0);
  fp8_pack(pf, sb, 4);
}

}  // namespace fa
