// Hardware-semantics probe for gfx950 (MI355X): verifies, on the device, every lane-layout
// assumption the attention kernels rely on.  Standalone: hipcc --offload-arch=gfx950 probe_gfx950.hip -o probe
// Prints PASS/FAIL per assumption and dumps raw lane data on failure.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <cmath>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(2);} } while (0)

// A: 32x16 row-major bf16, B: 16x32 row-major bf16 -> D 32x32 f32 using the ASSUMED layouts:
//  A operand: lane l holds A[l&31][8*(l>>5) + j], j=0..7
//  B operand: lane l holds B[8*(l>>5) + j][l&31]
//  D: reg r of lane l = D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31]
__global__ void mfma32_bf16(const __bf16* A, const __bf16* B, float* D) {
  int l = threadIdx.x, hi = l >> 5, c = l & 31;
  bf16x8 a, b;
  for (int j = 0; j < 8; ++j) { a[j] = A[c * 16 + 8 * hi + j]; b[j] = B[(8 * hi + j) * 32 + c]; }
  f32x16 acc = {};
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  for (int r = 0; r < 16; ++r) D[((r & 3) + 8 * (r >> 2) + 4 * hi) * 32 + c] = acc[r];
}
__global__ void mfma32_f16(const _Float16* A, const _Float16* B, float* D) {
  int l = threadIdx.x, hi = l >> 5, c = l & 31;
  f16x8 a, b;
  for (int j = 0; j < 8; ++j) { a[j] = A[c * 16 + 8 * hi + j]; b[j] = B[(8 * hi + j) * 32 + c]; }
  f32x16 acc = {};
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
  for (int r = 0; r < 16; ++r) D[((r & 3) + 8 * (r >> 2) + 4 * hi) * 32 + c] = acc[r];
}
// 16x16x32: A 16x32, B 32x16; lane l: A[l&15][8*(l>>4)+j], B[8*(l>>4)+j][l&15]; D reg r = D[4*(l>>4)+r][l&15]
__global__ void mfma16_bf16(const __bf16* A, const __bf16* B, float* D) {
  int l = threadIdx.x, g = l >> 4, c = l & 15;
  bf16x8 a, b;
  for (int j = 0; j < 8; ++j) { a[j] = A[c * 32 + 8 * g + j]; b[j] = B[(8 * g + j) * 16 + c]; }
  f32x4 acc = {};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  for (int r = 0; r < 4; ++r) D[(4 * g + r) * 16 + c] = acc[r];
}

// ds_read_b64_tr_b16: LDS holds M[r][c] = r*64 + c... we use a [8 rows][stride 72] short image with value = row*100+col.
// ASSUMPTION: within each 16-lane group, lane i supplies the address of (row i>>2, cols 4*(i&3)..+3) of a 4x16 block;
// the result in lane i, element j is M[j][i] of that block.
__global__ void tr_probe(short* out_hyp, short* out_raw) {
  __shared__ __attribute__((aligned(16))) short lds[64 * 72];
  int l = threadIdx.x;
  for (int i = l; i < 64 * 72; i += 64) lds[i] = (short)((i / 72) * 100 + (i % 72));
  __syncthreads();
  int g = l >> 4, i = l & 15;
  // hypothesis addressing: group g reads the 4x16 block at rows 4g..4g+3, cols 16*(g&1)..+15
  int row = 4 * g + (i >> 2), col = 16 * (g & 1) + 4 * (i & 3);
  s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds + row * 72 + col));
  for (int j = 0; j < 4; ++j) out_hyp[l * 4 + j] = v[j];
  // raw addressing: lane l reads 4 shorts at row l (value l*100 + 0..3) -> tells who gets what
  s16x4 w = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds + l * 72));
  for (int j = 0; j < 4; ++j) out_raw[l * 4 + j] = w[j];
}

__global__ void permlane_probe(unsigned* out) {
  unsigned l = threadIdx.x;
  unsigned a = 1000 + l, b = 2000 + l;
  auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  out[l] = r[0]; out[64 + l] = r[1];
  out[128 + l] = __shfl_xor((int)a, 32);
}

// bf16 conversion rounding: (__bf16)float must be round-to-nearest-even
__global__ void cvt_probe(const float* in, unsigned short* out, int n) {
  int t = threadIdx.x;
  if (t < n) { __bf16 x = (__bf16)in[t]; out[t] = *(unsigned short*)&x; }
}

// ---- FP8 (OCP e4m3) forms the fp8 forward (fa_fwd_fp8.hip) relies on
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(2))) int i32x2;
// v_mfma_scale_f32_32x32x64_f8f6f4, e4m3 A and B, unit scales.  A 32x64, B 64x32 row-major bytes; ASSUMED maps:
//   A: byte j of lane l = A[l&31][32*(l>>5) + j];  B: byte j of lane l = B[32*(l>>5) + j][l&31];  D as the bf16 form.
__global__ void mfma_scale_e4m3(const unsigned char* A, const unsigned char* B, float* D) {
  int l = threadIdx.x, hi = l >> 5, c = l & 31;
  i32x8 a, b;
  for (int w = 0; w < 8; ++w) {
    unsigned ua = 0, ub = 0;
    for (int t = 0; t < 4; ++t) { int j = 4 * w + t; ua |= (unsigned)A[c * 64 + 32 * hi + j] << (8 * t); ub |= (unsigned)B[(32 * hi + j) * 32 + c] << (8 * t); }
    a[w] = (int)ua; b[w] = (int)ub;
  }
  f32x16 acc = {};
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, 0, 0, 0, 127, 0, 127);
  for (int r = 0; r < 16; ++r) D[((r & 3) + 8 * (r >> 2) + 4 * hi) * 32 + c] = acc[r];
}
// The fp8 forward's P.V step: the accumulator tiles of P^T (lane = query q, register r of tile s = key 32 s + (r&3) + 8 (r>>2) + 4 (l>>5))
// packed with v_cvt_pk_fp8_f32 into the B operand, V^T as the A operand with byte j of lane (d, h) = V[32 (j>>4) + 8 ((j>>2)&3) + 4 h + (j&3)][d].
// P (32 queries x 64 keys) and V (64 keys x 32 columns) row-major floats, exactly representable in e4m3; O^T[d][q] out.
__global__ void pv_e4m3(const float* P, const unsigned char* V, float* OT) {
  int l = threadIdx.x, h = l >> 5, c = l & 31;
  i32x8 pf, vt;
  for (int s = 0; s < 2; ++s)
    for (int g = 0; g < 4; ++g) {
      float x[4];
      for (int t = 0; t < 4; ++t) { int r = 4 * g + t; x[t] = P[c * 64 + 32 * s + (r & 3) + 8 * (r >> 2) + 4 * h]; }
      int w = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
      pf[4 * s + g] = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], w, true);
    }
  for (int w = 0; w < 8; ++w) {
    unsigned u = 0;
    for (int t = 0; t < 4; ++t) { int j = 4 * w + t; u |= (unsigned)V[(32 * (j >> 4) + 8 * ((j >> 2) & 3) + 4 * h + (j & 3)) * 32 + c] << (8 * t); }
    vt[w] = (int)u;
  }
  f32x16 acc = {};
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vt, pf, acc, 0, 0, 0, 127, 0, 127);
  for (int r = 0; r < 16; ++r) OT[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + c] = acc[r];
}
// v_cvt_pk_fp8_f32: word_sel 0 writes bytes 0 (src0) and 1 (src1) and keeps bytes 2-3; word_sel 1 writes bytes 2 and 3 and keeps 0-1
__global__ void cvt_fp8_probe(const float* in, unsigned* out) {
  int t = threadIdx.x;
  if (t < 8) {
    out[2 * t] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(in[2 * t], in[2 * t + 1], (int)0xAABBCCDDu, false);
    out[2 * t + 1] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(in[2 * t], in[2 * t + 1], (int)0xAABBCCDDu, true);
  }
}
// ds_read_b64_tr_b8: ASSUMED, by analogy with the 16-bit form: inside each 16-lane group, lane i supplies the address of row i>>1,
// bytes 8*(i&1)..+7 of an 8 x 16 block of bytes, and receives column i (byte j = row j).
__global__ void tr8_probe(unsigned char* out) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * 128];
  int l = threadIdx.x;
  for (int i = l; i < 4 * 128; i += 64) lds[i] = (unsigned char)(i & 127);   // one 8 x 16 block per lane group, byte (r, c) = 16 r + c
  __syncthreads();
  int g = l >> 4, i = l & 15;
  i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2*)(lds + 128 * g + 8 * i));
  for (int j = 0; j < 8; ++j) out[l * 8 + j] = (unsigned char)(((unsigned)v[j >> 2] >> (8 * (j & 3))) & 0xFF);
}
// OCP e4m3 (bias 7, no infinities, 448 = largest finite), round to nearest even; |f| <= 448
static unsigned char f2e4m3(float f) {
  unsigned char s = f < 0 ? 0x80 : 0;
  float a = fabsf(f);
  if (a == 0.f) return s;
  int e;
  frexpf(a, &e);       // a = m 2^e, m in [0.5, 1)
  int E = e - 1 + 7;   // biased exponent of the 1.xxx form
  if (E < 1) return s | (unsigned char)rintf(a * 512.f);   // subnormal: k 2^-9 (k = 8 is the smallest normal, 0x08)
  float r = rintf((a / ldexpf(1.f, e - 1) - 1.f) * 8.f);
  if (r == 8.f) { r = 0.f; E += 1; }
  return s | (unsigned char)(E << 3) | (unsigned char)r;
}

static float bf2f(unsigned short b) { unsigned u = (unsigned)b << 16; float f; memcpy(&f, &u, 4); return f; }
static unsigned short f2bf(float f) { unsigned u; memcpy(&u, &f, 4); u += 0x7FFF + ((u >> 16) & 1); return (unsigned short)(u >> 16); }
static unsigned short f2h(float f) { _Float16 h = (_Float16)f; unsigned short s; memcpy(&s, &h, 2); return s; }

int main() {
  hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
  printf("device: %s arch %s CUs %d clock %d kHz LDS/block %zu regs/block %d L2 %d\n", prop.name, prop.gcnArchName,
         prop.multiProcessorCount, prop.clockRate, prop.sharedMemPerBlock, prop.regsPerBlock, prop.l2CacheSize);
  int fails = 0;
  srand(1);
  {  // mfma 32x32x16
    std::vector<float> A(32 * 16), B(16 * 32), Dref(32 * 32, 0.f);
    for (auto& x : A) x = (float)(rand() % 17 - 8);
    for (auto& x : B) x = (float)(rand() % 13 - 6);
    for (int m = 0; m < 32; ++m) for (int n = 0; n < 32; ++n) { float s = 0; for (int k = 0; k < 16; ++k) s += A[m * 16 + k] * B[k * 32 + n]; Dref[m * 32 + n] = s; }
    std::vector<unsigned short> Ab(32 * 16), Bb(16 * 32), Ah(32 * 16), Bh(16 * 32);
    for (int i = 0; i < 512; ++i) { Ab[i] = f2bf(A[i]); Bb[i] = f2bf(B[i]); Ah[i] = f2h(A[i]); Bh[i] = f2h(B[i]); }
    void *dA, *dB; float* dD; CK(hipMalloc(&dA, 1024)); CK(hipMalloc(&dB, 1024)); CK(hipMalloc(&dD, 4096));
    std::vector<float> D(1024);
    CK(hipMemcpy(dA, Ab.data(), 1024, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, Bb.data(), 1024, hipMemcpyHostToDevice));
    mfma32_bf16<<<1, 64>>>((const __bf16*)dA, (const __bf16*)dB, dD); CK(hipDeviceSynchronize());
    CK(hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost));
    int bad = 0; for (int i = 0; i < 1024; ++i) bad += (D[i] != Dref[i]);
    printf("[mfma_f32_32x32x16_bf16 layout] %s (%d mismatches)\n", bad ? "FAIL" : "PASS", bad); fails += bad != 0;
    CK(hipMemcpy(dA, Ah.data(), 1024, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, Bh.data(), 1024, hipMemcpyHostToDevice));
    mfma32_f16<<<1, 64>>>((const _Float16*)dA, (const _Float16*)dB, dD); CK(hipDeviceSynchronize());
    CK(hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost));
    bad = 0; for (int i = 0; i < 1024; ++i) bad += (D[i] != Dref[i]);
    printf("[mfma_f32_32x32x16_f16 layout] %s (%d mismatches)\n", bad ? "FAIL" : "PASS", bad); fails += bad != 0;
  }
  {  // mfma 16x16x32
    std::vector<float> A(16 * 32), B(32 * 16), Dref(256, 0.f);
    for (auto& x : A) x = (float)(rand() % 17 - 8);
    for (auto& x : B) x = (float)(rand() % 13 - 6);
    for (int m = 0; m < 16; ++m) for (int n = 0; n < 16; ++n) { float s = 0; for (int k = 0; k < 32; ++k) s += A[m * 32 + k] * B[k * 16 + n]; Dref[m * 16 + n] = s; }
    std::vector<unsigned short> Ab(512), Bb(512);
    for (int i = 0; i < 512; ++i) { Ab[i] = f2bf(A[i]); Bb[i] = f2bf(B[i]); }
    void *dA, *dB; float* dD; CK(hipMalloc(&dA, 1024)); CK(hipMalloc(&dB, 1024)); CK(hipMalloc(&dD, 1024));
    CK(hipMemcpy(dA, Ab.data(), 1024, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, Bb.data(), 1024, hipMemcpyHostToDevice));
    mfma16_bf16<<<1, 64>>>((const __bf16*)dA, (const __bf16*)dB, dD); CK(hipDeviceSynchronize());
    std::vector<float> D(256); CK(hipMemcpy(D.data(), dD, 1024, hipMemcpyDeviceToHost));
    int bad = 0; for (int i = 0; i < 256; ++i) bad += (D[i] != Dref[i]);
    printf("[mfma_f32_16x16x32_bf16 layout] %s (%d mismatches)\n", bad ? "FAIL" : "PASS", bad); fails += bad != 0;
  }
  {  // transpose read
    short *dh, *dr; CK(hipMalloc(&dh, 512)); CK(hipMalloc(&dr, 512));
    tr_probe<<<1, 64>>>(dh, dr); CK(hipDeviceSynchronize());
    std::vector<short> H(256), R(256);
    CK(hipMemcpy(H.data(), dh, 512, hipMemcpyDeviceToHost)); CK(hipMemcpy(R.data(), dr, 512, hipMemcpyDeviceToHost));
    int bad = 0;
    for (int l = 0; l < 64; ++l) for (int j = 0; j < 4; ++j) {
      int g = l >> 4, i = l & 15;
      int exp = (4 * g + j) * 100 + 16 * (g & 1) + i;
      bad += (H[l * 4 + j] != exp);
    }
    printf("[ds_read_b64_tr_b16 semantics] %s (%d mismatches)\n", bad ? "FAIL" : "PASS", bad); fails += bad != 0;
    printf("  raw tr dump (lane: 4 values; source value = srclane*100 + elem):\n");
    for (int l = 0; l < 64; ++l) { printf("  %2d: %5d %5d %5d %5d%s", l, R[l * 4], R[l * 4 + 1], R[l * 4 + 2], R[l * 4 + 3], (l & 3) == 3 ? "\n" : " |"); }
  }
  {  // permlane32_swap
    unsigned* d; CK(hipMalloc(&d, 192 * 4)); permlane_probe<<<1, 64>>>(d); CK(hipDeviceSynchronize());
    std::vector<unsigned> P(192); CK(hipMemcpy(P.data(), d, 768, hipMemcpyDeviceToHost));
    // assumption (guide T21): r[0] (vdst=a): lanes 0-31 keep a, lanes 32-63 get b from lane-32; r[1] (src=b): lanes 0-31 get a from lane+32, lanes 32-63 keep b
    int bad = 0;
    for (unsigned l = 0; l < 64; ++l) {
      unsigned e0 = l < 32 ? 1000 + l : 2000 + (l - 32);
      unsigned e1 = l < 32 ? 1000 + (l + 32) : 2000 + l;
      bad += (P[l] != e0) + (P[64 + l] != e1);
      bad += (P[128 + l] != 1000 + (l ^ 32));
    }
    printf("[permlane32_swap / shfl_xor 32 semantics] %s (%d mismatches)\n", bad ? "FAIL" : "PASS", bad); fails += bad != 0;
    if (bad) { for (int l = 0; l < 64; ++l) printf("  %2d: r0=%u r1=%u shfl=%u\n", l, P[l], P[64 + l], P[128 + l]); }
  }
  {  // bf16 RNE
    const int n = 8; float in[n] = {1.0f, 1.00390625f, 1.01171875f, 3.1415926f, -2.7182817f, 65504.f, 1e-8f, 0.3333333f};
    float* di; unsigned short* dout; CK(hipMalloc(&di, 64)); CK(hipMalloc(&dout, 32));
    CK(hipMemcpy(di, in, n * 4, hipMemcpyHostToDevice)); cvt_probe<<<1, 64>>>(di, dout, n); CK(hipDeviceSynchronize());
    unsigned short o[n]; CK(hipMemcpy(o, dout, n * 2, hipMemcpyDeviceToHost));
    int bad = 0; for (int i = 0; i < n; ++i) bad += (o[i] != f2bf(in[i]));
    printf("[float->bf16 is RNE] %s (%d mismatches)\n", bad ? "FAIL" : "PASS", bad); fails += bad != 0;
  }
  {  // scaled fp8 MFMA: A / B / D maps on exact integer data, asymmetric B
    std::vector<float> A(32 * 64), B(64 * 32), Dref(32 * 32, 0.f);
    for (auto& x : A) x = (float)(rand() % 17 - 8);
    for (int kk = 0; kk < 64; ++kk) for (int n = 0; n < 32; ++n) B[kk * 32 + n] = (float)((kk * 7 + n * 3) % 13 - 6) + (n > kk % 32 ? 0.5f : 0.f);
    for (int m = 0; m < 32; ++m) for (int n = 0; n < 32; ++n) { float s = 0; for (int kk = 0; kk < 64; ++kk) s += A[m * 64 + kk] * B[kk * 32 + n]; Dref[m * 32 + n] = s; }
    std::vector<unsigned char> A8(2048), B8(2048);
    for (int i = 0; i < 2048; ++i) { A8[i] = f2e4m3(A[i]); B8[i] = f2e4m3(B[i]); }
    unsigned char *dA, *dB; float* dD; CK(hipMalloc(&dA, 2048)); CK(hipMalloc(&dB, 2048)); CK(hipMalloc(&dD, 4096));
    CK(hipMemcpy(dA, A8.data(), 2048, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, B8.data(), 2048, hipMemcpyHostToDevice));
    mfma_scale_e4m3<<<1, 64>>>(dA, dB, dD); CK(hipDeviceSynchronize());
    std::vector<float> D(1024); CK(hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost));
    int bad = 0; for (int i = 0; i < 1024; ++i) bad += (D[i] != Dref[i]);
    printf("[mfma_scale_f32_32x32x64_f8f6f4 e4m3 A/B/D maps] %s (%d mismatches)\n", bad ? "FAIL" : "PASS", bad); fails += bad != 0;
    // the P.V step of the fp8 forward: accumulator-layout P^T packed by v_cvt_pk_fp8_f32, V^T in the permuted key order
    std::vector<float> P(32 * 64), V(64 * 32), OT(32 * 32, 0.f);
    const float pv[8] = {0.f, 1.f, 0.5f, 2.f, 0.25f, 3.f, 1.5f, 0.125f};
    for (int i = 0; i < 2048; ++i) { P[i] = pv[rand() % 8]; V[i] = (float)(rand() % 15 - 7); }
    for (int d = 0; d < 32; ++d) for (int q = 0; q < 32; ++q) { float s = 0; for (int kk = 0; kk < 64; ++kk) s += V[kk * 32 + d] * P[q * 64 + kk]; OT[d * 32 + q] = s; }
    std::vector<unsigned char> V8(2048);
    for (int i = 0; i < 2048; ++i) V8[i] = f2e4m3(V[i]);
    float* dP; CK(hipMalloc(&dP, 8192));
    CK(hipMemcpy(dP, P.data(), 8192, hipMemcpyHostToDevice)); CK(hipMemcpy(dA, V8.data(), 2048, hipMemcpyHostToDevice));
    pv_e4m3<<<1, 64>>>(dP, dA, dD); CK(hipDeviceSynchronize());
    CK(hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost));
    bad = 0; for (int i = 0; i < 1024; ++i) bad += (D[i] != OT[i]);
    printf("[fp8 forward P.V step: cvt_pk_fp8 P^T as B, permuted V^T as A] %s (%d mismatches)\n", bad ? "FAIL" : "PASS", bad); fails += bad != 0;
  }
  {  // v_cvt_pk_fp8_f32 byte placement and rounding (OCP e4m3, RNE)
    const float in[16] = {1.f, 2.f, -1.f, 448.f, 0.5f, 3.f, 1.0625f, 1.1875f, 0.001953125f, -0.0009765625f, 240.f, 1e-12f, 13.f, -0.3f, 100.f, 0.0178f};
    float* di; unsigned* dout; CK(hipMalloc(&di, 64)); CK(hipMalloc(&dout, 64));
    CK(hipMemcpy(di, in, 64, hipMemcpyHostToDevice)); cvt_fp8_probe<<<1, 64>>>(di, dout); CK(hipDeviceSynchronize());
    unsigned o[16]; CK(hipMemcpy(o, dout, 64, hipMemcpyDeviceToHost));
    int bad = 0;
    for (int t = 0; t < 8; ++t) {
      const unsigned lo = f2e4m3(in[2 * t]) | ((unsigned)f2e4m3(in[2 * t + 1]) << 8);
      bad += (o[2 * t] != (0xAABB0000u | lo)) + (o[2 * t + 1] != ((lo << 16) | 0xCCDDu));
    }
    printf("[v_cvt_pk_fp8_f32 byte placement / e4m3 RNE] %s (%d mismatches)\n", bad ? "FAIL" : "PASS", bad); fails += bad != 0;
    if (bad) for (int t = 0; t < 8; ++t) printf("  (%g, %g): word_sel 0 -> %08x, 1 -> %08x\n", in[2 * t], in[2 * t + 1], o[2 * t], o[2 * t + 1]);
  }
  {  // ds_read_b64_tr_b8
    unsigned char* d; CK(hipMalloc(&d, 512)); tr8_probe<<<1, 64>>>(d); CK(hipDeviceSynchronize());
    unsigned char R[512]; CK(hipMemcpy(R, d, 512, hipMemcpyDeviceToHost));
    int bad = 0;
    for (int l = 0; l < 64; ++l) for (int j = 0; j < 8; ++j) bad += (R[l * 8 + j] != (unsigned char)(16 * j + (l & 15)));
    printf("[ds_read_b64_tr_b8 lane map] %s (%d mismatches)\n", bad ? "FAIL" : "PASS", bad); fails += bad != 0;
    if (bad) for (int l = 0; l < 16; ++l) printf("  %2d: %3d %3d %3d %3d %3d %3d %3d %3d\n", l, R[l * 8], R[l * 8 + 1], R[l * 8 + 2], R[l * 8 + 3], R[l * 8 + 4], R[l * 8 + 5], R[l * 8 + 6], R[l * 8 + 7]);
  }
  printf("PROBE %s\n", fails ? "FAILED" : "ALL PASS");
  return fails ? 1 : 0;
}
