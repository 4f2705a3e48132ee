// libfa_gfx950_combine.so (include/fa_gfx950_combine.h): the merge of partial attention results (o_i, lse_i) over disjoint key sets,
//     lse = m + log(sum_live exp(lse_i - m)),  out = sum_live exp(lse_i - lse) * o_i,
// with this project's convention for empty partials built in (a non-finite lse: weight 0, the o row is not fetched).  HBM-bound: a lane owns a CHUNK of 8
// consecutive channels of a row -- one 16-byte load per 16-bit partial, two per fp32 partial, 16-byte stores -- and keeps several partials in flight.
//
// Two kernels, picked from the shapes alone (never from strides or values: the bits of a result do not depend on the layout):
//   rows     many rows, few partials (the prefill merge).  A row takes lpr = d / 8 lanes; a wave holds 64 / lpr whole rows, so a row never straddles waves and
//            the in-place lse store follows every load of that lse in its own wave.  Every lane computes its row's weights itself from the row's n lse values
//            (same-address loads within a row): for n <= 8 that is cheaper than a shuffle pattern that changes with lpr.  Partials are added in split order.
//   splits   few rows, many partials (the decode combine).  One workgroup per row: thread t reads lse_t, the workgroup's maximum and sum give the weights once,
//            shared through LDS; split i goes to slot i % slots (a slot is lpr threads), every slot adds its partials in split order with 8 loads in flight,
//            and the slots are added through LDS in slot order.
// The o dtype of a source and of the output is a run-time field: the branches on it are wave-uniform, and one instantiation per kernel keeps the library small.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/fa_gfx950_combine.h"

namespace fc {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kMaxSlots = 32;        // of the splits kernel: the last, serial sum over the slots stays short
constexpr int kRowsInFlight = 4;     // partial loads in flight per lane: rows kernel (many waves per SIMD hide the rest)
constexpr int kSplitsInFlight = 8;   // ... splits kernel (few workgroups)

struct Src {   // device view of one FaCombineSource: o strides in BYTES, lse strides in elements
  const char* o;
  const float* lse;
  int64_t o_ss, o_bs, o_rs, o_hs, l_ss, l_bs, l_rs, l_hs;
  int32_t n, dt;
};

struct CombineK {
  Src src[FA_COMBINE_MAX_SOURCES];   // (an absent source 1 has n = 0)
  char* out;
  float* lse;                        // may be null
  int64_t out_bs, out_rs, out_hs, l_bs, l_rs, l_hs;
  uint32_t rows, s, h;
  int32_t n, out_dt, lpr, rpw, slots;
  float empty_lse;
};

struct Raw { u32x4 a, b; };   // a chunk as loaded: 8 16-bit elements in a, or 8 fp32 in a, b

__device__ __forceinline__ bool live(float lse) { return fabsf(lse) < INFINITY; }

__device__ __forceinline__ Raw load_chunk(const char* p, int dt) {
  Raw r;
  r.a = *reinterpret_cast<const u32x4*>(p);
  r.b = u32x4{0u, 0u, 0u, 0u};
  if (dt == FA_COMBINE_DTYPE_FP32) r.b = *reinterpret_cast<const u32x4*>(p + 16);
  return r;
}

// acc += w * chunk
__device__ __forceinline__ void fma_chunk(float (&acc)[8], float w, const Raw& r, int dt) {
  float v[8];
  if (dt == FA_COMBINE_DTYPE_FP32) {
    const f32x4 lo = __builtin_bit_cast(f32x4, r.a), hi = __builtin_bit_cast(f32x4, r.b);   // (whole vectors: a bit_cast of ONE vector element reads element 0)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = lo[j];
      v[4 + j] = hi[j];
    }
  } else if (dt == FA_COMBINE_DTYPE_BF16) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = __builtin_bit_cast(float, r.a[j] << 16);
      v[2 * j + 1] = __builtin_bit_cast(float, r.a[j] & 0xffff0000u);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = (float)__builtin_bit_cast(_Float16, (uint16_t)(r.a[j] & 0xffffu));
      v[2 * j + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(r.a[j] >> 16));
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, v[j], acc[j]);
}

// the one rounding to the output dtype (round to nearest even), 16-byte stores
__device__ __forceinline__ void store_chunk(char* p, int dt, const float (&acc)[8]) {
  if (dt == FA_COMBINE_DTYPE_FP32) {
    *reinterpret_cast<u32x4*>(p) = __builtin_bit_cast(u32x4, f32x4{acc[0], acc[1], acc[2], acc[3]});
    *reinterpret_cast<u32x4*>(p + 16) = __builtin_bit_cast(u32x4, f32x4{acc[4], acc[5], acc[6], acc[7]});
    return;
  }
  u32x4 w;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t e0, e1;
    if (dt == FA_COMBINE_DTYPE_BF16) {
      e0 = __builtin_bit_cast(uint16_t, (__bf16)acc[2 * j]);
      e1 = __builtin_bit_cast(uint16_t, (__bf16)acc[2 * j + 1]);
    } else {
      e0 = __builtin_bit_cast(uint16_t, (_Float16)acc[2 * j]);
      e1 = __builtin_bit_cast(uint16_t, (_Float16)acc[2 * j + 1]);
    }
    w[j] = e0 | (e1 << 16);
  }
  *reinterpret_cast<u32x4*>(p) = w;
}

// The places of one row (and one chunk of it) in every tensor of the call.
struct Place {
  const char* o[FA_COMBINE_MAX_SOURCES];
  const float* l[FA_COMBINE_MAX_SOURCES];
  char* out;
  float* lse;
};

__device__ __forceinline__ Place place_of(const CombineK& p, uint32_t row, int dc) {
  const uint32_t h = row % p.h, t = row / p.h;
  const int64_t hh = h, ss = t % p.s, bb = t / p.s;
  Place pl;
#pragma unroll
  for (int k = 0; k < FA_COMBINE_MAX_SOURCES; ++k) {
    const Src& s = p.src[k];
    pl.o[k] = s.o + bb * s.o_bs + ss * s.o_rs + hh * s.o_hs + (int64_t)dc * (s.dt == FA_COMBINE_DTYPE_FP32 ? 32 : 16);
    pl.l[k] = s.lse + bb * s.l_bs + ss * s.l_rs + hh * s.l_hs;
  }
  pl.out = p.out + bb * p.out_bs + ss * p.out_rs + hh * p.out_hs + (int64_t)dc * (p.out_dt == FA_COMBINE_DTYPE_FP32 ? 32 : 16);
  pl.lse = p.lse ? p.lse + bb * p.l_bs + ss * p.l_rs + hh * p.l_hs : nullptr;
  return pl;
}

__device__ __forceinline__ float lse_at(const CombineK& p, const Place& pl, int i) {
  const int n0 = p.src[0].n;
  return i < n0 ? pl.l[0][(int64_t)i * p.src[0].l_ss] : pl.l[1][(int64_t)(i - n0) * p.src[1].l_ss];
}
__device__ __forceinline__ const char* o_at(const CombineK& p, const Place& pl, int i) {
  const int n0 = p.src[0].n;
  return i < n0 ? pl.o[0] + (int64_t)i * p.src[0].o_ss : pl.o[1] + (int64_t)(i - n0) * p.src[1].o_ss;
}
__device__ __forceinline__ int dt_at(const CombineK& p, int i) { return i < p.src[0].n ? p.src[0].dt : p.src[1].dt; }

// acc += sum of w_i * o_i over the splits first, first + step, ... < n, in that order, F loads in flight; a zero weight skips the load.
template <int F, typename W>
__device__ __forceinline__ void accumulate(float (&acc)[8], const CombineK& p, const Place& pl, int first, int step, W weight) {
  for (int i0 = first; i0 < p.n; i0 += F * step) {
    Raw r[F];
    float w[F];
#pragma unroll
    for (int j = 0; j < F; ++j) {
      const int i = i0 + j * step;
      w[j] = i < p.n ? weight(i) : 0.f;
      r[j].a = r[j].b = u32x4{0u, 0u, 0u, 0u};
      if (w[j] != 0.f) r[j] = load_chunk(o_at(p, pl, i), dt_at(p, i));
    }
#pragma unroll
    for (int j = 0; j < F; ++j) fma_chunk(acc, w[j], r[j], dt_at(p, min(i0 + j * step, p.n - 1)));
  }
}

// grid: ceil(rows / rpw) waves, 4 per workgroup.
__global__ void __launch_bounds__(kThreads) fa_combine_rows_kernel(const CombineK p) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const int rw = lane / p.lpr, dc = lane - rw * p.lpr;
  const uint64_t row64 = (uint64_t)wave * p.rpw + rw;
  if (rw >= p.rpw || row64 >= p.rows) return;
  const Place pl = place_of(p, (uint32_t)row64, dc);
  float m = -INFINITY;
  for (int i = 0; i < p.n; ++i) {
    const float l = lse_at(p, pl, i);
    if (live(l)) m = fmaxf(m, l);
  }
  const bool dead = m == -INFINITY;
  float sum = 0.f;
  if (!dead)
    for (int i = 0; i < p.n; ++i) {
      const float l = lse_at(p, pl, i);
      if (live(l)) sum += expf(l - m);
    }
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (!dead)
    accumulate<kRowsInFlight>(acc, p, pl, 0, 1, [&](int i) {
      const float l = lse_at(p, pl, i);
      return live(l) ? expf(l - m) / sum : 0.f;
    });
  store_chunk(pl.out, p.out_dt, acc);
  if (dc == 0 && pl.lse) *pl.lse = dead ? p.empty_lse : m + logf(sum);
}

// workgroup sum / maximum of one float per thread in a fixed order, returned to every thread
template <bool MAX>
__device__ __forceinline__ float block_reduce(float x, float* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float y = __shfl_xor(x, o, 64);
    x = MAX ? fmaxf(x, y) : x + y;
  }
  __syncthreads();   // (the previous use of lds is over)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
  __syncthreads();
  return MAX ? fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3])) : (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// grid: one workgroup per row.
__global__ void __launch_bounds__(kThreads) fa_combine_splits_kernel(const CombineK p) {
  __shared__ float red4[4];
  __shared__ float wts[FA_COMBINE_MAX_SPLITS];
  __shared__ __attribute__((aligned(16))) float part[kThreads * 8];
  const int t = threadIdx.x;
  const int slot = t / p.lpr, dc = t - slot * p.lpr;
  const Place pl = place_of(p, blockIdx.x, slot < p.slots ? dc : 0);
  const float l = t < p.n ? lse_at(p, pl, t) : -INFINITY;
  const bool alive = live(l);
  const float m = block_reduce<true>(alive ? l : -INFINITY, red4);
  const bool dead = m == -INFINITY;
  const float e = alive ? expf(l - m) : 0.f;
  const float sum = block_reduce<false>(e, red4);
  wts[t] = alive ? e / sum : 0.f;
  __syncthreads();
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (slot < p.slots && !dead) accumulate<kSplitsInFlight>(acc, p, pl, slot, p.slots, [&](int i) { return wts[i]; });
  f32x4* mine = reinterpret_cast<f32x4*>(part + t * 8);
  mine[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
  mine[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
  __syncthreads();
  if (t >= p.lpr) return;
  for (int k = 1; k < p.slots; ++k) {   // slot 0 (this thread's own acc) + slot 1 + ...
    const float* other = part + (k * p.lpr + t) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += other[j];
  }
  store_chunk(pl.out, p.out_dt, acc);
  if (t == 0 && pl.lse) *pl.lse = dead ? p.empty_lse : m + logf(sum);
}

}  // namespace fc

// ---------------------------------------------------------------- host side: validation and the launch ----------------------------------------------------------------
namespace {

enum { kOk = 0, kInvalid = -1, kUnsupported = -2, kLaunch = -3 };   // FA_OK / FA_ERR_* of include/fa_gfx950.h

thread_local char g_err[512] = {0};
thread_local const char* g_kernel = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

const char* const kFn = "fa_combine";

int elem_size(int dt) { return dt == FA_COMBINE_DTYPE_FP32 ? 4 : dt == FA_COMBINE_DTYPE_FP16 || dt == FA_COMBINE_DTYPE_BF16 ? 2 : 0; }

// One stride of an o tensor, in elements of `esz` bytes; a dimension of one element may have any stride.
int check_o_stride(const char* tensor, const char* what, int64_t stride, int64_t extent, int esz, bool output) {
  if (extent <= 1) return kOk;
  if ((stride * esz) % 16 != 0)
    return fail(kInvalid, "%s: %s: %s stride %lld (elements of %d bytes) must be a multiple of 16 bytes", kFn, tensor, what, (long long)stride, esz);
  if (output && stride == 0) return fail(kInvalid, "%s: %s: %s stride of an output must not be 0", kFn, tensor, what);
  return kOk;
}

int check_lse_out_stride(const char* what, int64_t stride, int64_t extent) {
  if (extent > 1 && stride == 0) return fail(kInvalid, "%s: lse: %s stride of an output must not be 0", kFn, what);
  return kOk;
}

}  // namespace

extern "C" {

int fa_combine_abi_version(void) { return FA_COMBINE_ABI_VERSION; }
int fa_sizeof_combine_source(void) { return (int)sizeof(FaCombineSource); }
int fa_sizeof_combine_params(void) { return (int)sizeof(FaCombineParams); }
const char* fa_combine_last_error(void) { return g_err; }
const char* fa_combine_last_kernel_name(void) { return g_kernel; }

int fa_combine(const FaCombineParams* a, void* stream) {
  g_kernel = "";
  if (!a) return fail(kInvalid, "%s: params is NULL", kFn);
  g_err[0] = 0;
  static const char* const kO[FA_COMBINE_MAX_SOURCES] = {"src[0].o", "src[1].o"};
  static const char* const kL[FA_COMBINE_MAX_SOURCES] = {"src[0].lse", "src[1].lse"};
  if (a->n_sources < 1 || a->n_sources > FA_COMBINE_MAX_SOURCES) return fail(kInvalid, "%s: n_sources = %d: one call takes 1 to %d sources", kFn, a->n_sources, FA_COMBINE_MAX_SOURCES);
  int64_t n = 0;
  for (int k = 0; k < a->n_sources; ++k) {
    if (a->src[k].n_splits < 1) return fail(kInvalid, "%s: src[%d].n_splits = %d must be at least 1", kFn, k, a->src[k].n_splits);
    if (!elem_size(a->src[k].dtype)) return fail(kInvalid, "%s: src[%d].dtype must be fp16 (0), bf16 (1) or fp32 (3)", kFn, k);
    n += a->src[k].n_splits;
  }
  if (n > FA_COMBINE_MAX_SPLITS) return fail(kInvalid, "%s: n_splits: %lld partials over all sources exceed FA_COMBINE_MAX_SPLITS = %d", kFn, (long long)n, FA_COMBINE_MAX_SPLITS);
  if (!elem_size(a->out_dtype)) return fail(kInvalid, "%s: out_dtype must be fp16 (0), bf16 (1) or fp32 (3)", kFn);
  if (a->b < 0 || a->s < 0 || a->h < 0) return fail(kInvalid, "%s: b, s and h must not be negative", kFn);
  if (a->d < 8 || a->d > 512 || a->d % 8 != 0) return fail(kInvalid, "%s: d = %d: the head dimension must be a multiple of 8 in [8, 512]", kFn, a->d);
  if (a->empty_lse_sign != 1 && a->empty_lse_sign != -1) return fail(kInvalid, "%s: empty_lse_sign must be +1 or -1", kFn);
  if (a->path < FA_COMBINE_PATH_AUTO || a->path > FA_COMBINE_PATH_SPLITS) return fail(kInvalid, "%s: path must be 0 (automatic), 1 (rows kernel) or 2 (splits kernel)", kFn);
  if (a->b == 0 || a->s == 0 || a->h == 0) return kOk;
  if ((int64_t)a->b * a->s > INT32_MAX || (int64_t)a->b * a->s * a->h > INT32_MAX) return fail(kInvalid, "%s: b * s * h must be below 2^31", kFn);
  const int64_t rows = (int64_t)a->b * a->s * a->h;
  int rc;
  for (int k = 0; k < a->n_sources; ++k) {
    const FaCombineSource& s = a->src[k];
    const int esz = elem_size(s.dtype);
    if (!s.o) return fail(kInvalid, "%s: %s must be non-NULL", kFn, kO[k]);
    if (!s.lse) return fail(kInvalid, "%s: %s must be non-NULL", kFn, kL[k]);
    if (((uintptr_t)s.o & 15u) != 0) return fail(kInvalid, "%s: %s must be 16-byte aligned", kFn, kO[k]);
    if (((uintptr_t)s.lse & 3u) != 0) return fail(kInvalid, "%s: %s must be 4-byte aligned", kFn, kL[k]);
    if ((rc = check_o_stride(kO[k], "split", s.o_split_stride, s.n_splits, esz, false)) || (rc = check_o_stride(kO[k], "batch", s.o_batch_stride, a->b, esz, false)) ||
        (rc = check_o_stride(kO[k], "row", s.o_row_stride, a->s, esz, false)) || (rc = check_o_stride(kO[k], "head", s.o_head_stride, a->h, esz, false)))
      return rc;
  }
  {
    const int esz = elem_size(a->out_dtype);
    if (!a->out) return fail(kInvalid, "%s: out must be non-NULL", kFn);
    if (((uintptr_t)a->out & 15u) != 0) return fail(kInvalid, "%s: out must be 16-byte aligned", kFn);
    if (((uintptr_t)a->lse & 3u) != 0) return fail(kInvalid, "%s: lse must be 4-byte aligned", kFn);
    if ((rc = check_o_stride("out", "batch", a->out_batch_stride, a->b, esz, true)) || (rc = check_o_stride("out", "row", a->out_row_stride, a->s, esz, true)) ||
        (rc = check_o_stride("out", "head", a->out_head_stride, a->h, esz, true)))
      return rc;
    if (a->lse && ((rc = check_lse_out_stride("batch", a->lse_batch_stride, a->b)) || (rc = check_lse_out_stride("row", a->lse_row_stride, a->s)) ||
                   (rc = check_lse_out_stride("head", a->lse_head_stride, a->h))))
      return rc;
  }

  fc::CombineK k{};
  for (int i = 0; i < a->n_sources; ++i) {
    const FaCombineSource& s = a->src[i];
    const int esz = elem_size(s.dtype);
    fc::Src& d = k.src[i];
    d.o = (const char*)s.o; d.lse = s.lse;
    d.o_ss = s.o_split_stride * esz; d.o_bs = s.o_batch_stride * esz; d.o_rs = s.o_row_stride * esz; d.o_hs = s.o_head_stride * esz;
    d.l_ss = s.lse_split_stride; d.l_bs = s.lse_batch_stride; d.l_rs = s.lse_row_stride; d.l_hs = s.lse_head_stride;
    d.n = s.n_splits; d.dt = s.dtype;
  }
  if (a->n_sources == 1) { k.src[1] = k.src[0]; k.src[1].n = 0; }   // (never indexed: every split is below src[0].n)
  const int osz = elem_size(a->out_dtype);
  k.out = (char*)a->out; k.lse = a->lse;
  k.out_bs = a->out_batch_stride * osz; k.out_rs = a->out_row_stride * osz; k.out_hs = a->out_head_stride * osz;
  k.l_bs = a->lse_batch_stride; k.l_rs = a->lse_row_stride; k.l_hs = a->lse_head_stride;
  k.rows = (uint32_t)rows; k.s = (uint32_t)a->s; k.h = (uint32_t)a->h;
  k.n = (int)n; k.out_dt = a->out_dtype;
  k.lpr = a->d / 8;
  k.rpw = 64 / k.lpr;
  k.slots = (int)std::min<int64_t>(std::min(fc::kMaxSlots, fc::kThreads / k.lpr), n);
  k.empty_lse = a->empty_lse_sign > 0 ? INFINITY : -INFINITY;
  // Shapes only.  The rows kernel fills the chip from 256 CUs x 4 waves of rows on; below that, and with partials to share out, a workgroup per row does.
  const int64_t row_waves = (rows + k.rpw - 1) / k.rpw;
  const bool splits = a->path == FA_COMBINE_PATH_SPLITS ||
                      (a->path == FA_COMBINE_PATH_AUTO && (n > FA_COMBINE_ROWS_MAX_SPLITS || (n >= 4 && row_waves < 1024)));
  hipStream_t st = (hipStream_t)stream;
  if (splits) {
    g_kernel = "fa_combine_splits_kernel";
    hipLaunchKernelGGL(fc::fa_combine_splits_kernel, dim3((unsigned)rows), dim3(fc::kThreads), 0, st, k);
  } else {
    g_kernel = "fa_combine_rows_kernel";
    hipLaunchKernelGGL(fc::fa_combine_rows_kernel, dim3((unsigned)((row_waves + 3) / 4)), dim3(fc::kThreads), 0, st, k);
  }
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    g_kernel = "";
    return fail(kLaunch, "%s: launch failed: %s", kFn, hipGetErrorString(e));
  }
  return kOk;
}

}  // extern "C"
