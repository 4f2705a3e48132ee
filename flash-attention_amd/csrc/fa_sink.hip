// libfa_gfx950_sink.so (include/fa_gfx950_sink.h): learnable attention sinks as a post-pass over (out, lse),
//     lse' = max(lse, s) + log1p(exp(-|lse - s|)),  out' = out / (1 + exp(s - lse)),  dsink[h] = - sum_rows exp(s_h - lse') * softmax_d,
// with this project's convention for rows without a visible key built in (a non-finite lse: out' = 0 and the out row is not fetched, lse' = s, lse_bwd = +inf;
// the dsink sum skips the row and does not fetch its softmax_d).  Both kernels are HBM-bound.
//
//   apply    out rows are (b, s, h, :) and lse is (b, h, s): a workgroup owns a TILE of 64 rows of one batch entry, TS consecutive sequence positions times
//            TH = 64 / TS consecutive heads, TS = min(64, next power of two of s).  Wave 0 reads the tile's 64 lse values with lane = (head, position), position
//            fastest -- runs of TS consecutive floats, one 256-byte line per head for s >= 64, and for a decode step (s = 1) 64 consecutive heads -- computes the
//            row's factor and lse' ONCE, stores lse' / lse_bwd the same way and leaves the factors in LDS.  Then all four waves move the tile's out rows, a lane
//            owning a CHUNK of 8 consecutive channels (16-byte loads and stores; up to 4 in flight: 4 at d >= 128, 2 at d = 64, 1 below d = 40), rows taken position-major so that a tile of many heads (decode)
//            is one contiguous run.  The LDS slot alternates between tiles: one barrier per tile.  The grid is capped at 8 workgroups per CU and strides.
//   dsink    nblk = min(64, ceil(b * s / 1024)) workgroups per head, from the shapes alone; workgroup i takes rows i * 256 + t, + nblk * 256, ... (consecutive
//            threads on consecutive positions), adds them in that order per thread, then the threads in a fixed tree, and stores one partial; the second kernel
//            adds a head's partials in one wave, again a fixed tree.  No atomics: the bits of dsink are the same on every run.
// The dtypes are run-time fields: the branches on them are wave-uniform, and one instantiation per kernel keeps the library small.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/fa_gfx950_sink.h"

namespace fs {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kTileRows = 64;        // rows of a tile of the apply kernel: one per lane of wave 0
constexpr int kInFlight = 4;         // 16-byte loads in flight per lane at most: 64 rows / (256 / (d / 8)) rows per pass, so 4 only from d = 128
constexpr int kBlocksPerCU = 8, kCUs = 256;
constexpr int kDsinkRowsPerBlock = 1024;
constexpr float kNoRow = -1.f;       // LDS marker of a tile slot past the end of s or h (a factor is in [0, 1])

struct ApplyK {
  const char* out_in;
  const float* lse_in;
  const char* sink;
  char* out;
  float* lse;
  float* lse_bwd;                    // may be null
  int64_t oi_bs, oi_rs, oi_hs, o_bs, o_rs, o_hs;                               // BYTES
  int64_t li_bs, li_rs, li_hs, l_bs, l_rs, l_hs, lb_bs, lb_rs, lb_hs, sink_st;   // elements
  uint32_t s, h, tiles_s, tiles_h, tiles;
  int32_t ts_log2, lpr, rpp, dt, sink_dt;
};

struct DsinkK {
  const float* d;
  const float* l;
  const char* sink;
  float* dsink;
  float* ws;
  int64_t d_bs, d_rs, d_hs, l_bs, l_rs, l_hs, sink_st, dsink_st;
  uint32_t rows, s;
  int32_t nblk, sink_dt;
};

__device__ __forceinline__ bool live(float lse) { return fabsf(lse) < INFINITY; }

__device__ __forceinline__ float load_sink(const char* p, int64_t i, int dt) {
  if (dt == FA_SINK_DTYPE_FP32) return reinterpret_cast<const float*>(p)[i];
  const uint16_t bits = reinterpret_cast<const uint16_t*>(p)[i];
  return dt == FA_SINK_DTYPE_BF16 ? __builtin_bit_cast(float, (uint32_t)bits << 16) : (float)__builtin_bit_cast(_Float16, bits);
}

// chunk * f with the one rounding to the dtype (round to nearest even)
__device__ __forceinline__ u32x4 scale_chunk(const u32x4 r, float f, int dt) {
  u32x4 w;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t e0, e1;
    if (dt == FA_SINK_DTYPE_BF16) {
      const float lo = __builtin_bit_cast(float, r[j] << 16), hi = __builtin_bit_cast(float, r[j] & 0xffff0000u);
      e0 = __builtin_bit_cast(uint16_t, (__bf16)(lo * f));
      e1 = __builtin_bit_cast(uint16_t, (__bf16)(hi * f));
    } else {
      const float lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(r[j] & 0xffffu)), hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(r[j] >> 16));
      e0 = __builtin_bit_cast(uint16_t, (_Float16)(lo * f));
      e1 = __builtin_bit_cast(uint16_t, (_Float16)(hi * f));
    }
    w[j] = e0 | (e1 << 16);
  }
  return w;
}

// grid: min(tiles, 8 per CU) workgroups, striding over the tiles.
__global__ void __launch_bounds__(kThreads) fa_sink_apply_kernel(const ApplyK p) {
  __shared__ float factor[2][kTileRows];
  const int t = threadIdx.x;
  const int r0 = t / p.lpr, dc = t - r0 * p.lpr;
  const bool mover = r0 < p.rpp;                       // (d = 40: 5 lanes per row, 51 rows per pass, one idle thread)
  const uint32_t ts_mask = (1u << p.ts_log2) - 1u, th_log2 = 6 - p.ts_log2, th_mask = (1u << th_log2) - 1u;
  int slot = 0;
  for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x, slot ^= 1) {
    const uint32_t th = tile % p.tiles_h, rest = tile / p.tiles_h;
    const uint32_t s0 = (rest % p.tiles_s) << p.ts_log2, h0 = th << th_log2;
    const int64_t bb = rest / p.tiles_s;
    if (t < kTileRows) {                               // lane = (head, position), position fastest
      const uint32_t ss = s0 + ((uint32_t)t & ts_mask), hh = h0 + ((uint32_t)t >> p.ts_log2);
      float f = kNoRow;
      if (ss < p.s && hh < p.h) {
        const float l = p.lse_in[bb * p.li_bs + (int64_t)ss * p.li_rs + (int64_t)hh * p.li_hs];
        const float sv = load_sink(p.sink, (int64_t)hh * p.sink_st, p.sink_dt);
        float l2, lb;
        if (sv == -INFINITY) {                         // no sink: the identity, a row without a key keeps its marker
          f = live(l) ? 1.f : 0.f;
          l2 = l;
          lb = live(l) ? l : INFINITY;
        } else if (!live(l)) {                         // no visible key: everything sits on the sink
          f = 0.f;
          l2 = sv;
          lb = INFINITY;
        } else {
          f = 1.f / (1.f + expf(sv - l));              // (expf(+large) = inf -> 0; expf(-large) = 0 -> 1)
          l2 = fmaxf(l, sv) + log1pf(expf(-fabsf(l - sv)));
          lb = l2;
        }
        p.lse[bb * p.l_bs + (int64_t)ss * p.l_rs + (int64_t)hh * p.l_hs] = l2;
        if (p.lse_bwd) p.lse_bwd[bb * p.lb_bs + (int64_t)ss * p.lb_rs + (int64_t)hh * p.lb_hs] = lb;
      }
      factor[slot][t] = f;
    }
    __syncthreads();                                   // (the slot two tiles back is free: every wave passed the barrier in between after reading it)
    if (!mover) continue;
    for (int e0 = r0; e0 < kTileRows; e0 += kInFlight * p.rpp) {
      u32x4 raw[kInFlight];
      float f[kInFlight];
      int64_t off_in[kInFlight], off_out[kInFlight];
#pragma unroll
      for (int j = 0; j < kInFlight; ++j) {            // row e of the tile, position-major: (position, head) = (e / TH, e % TH)
        const int e = e0 + j * p.rpp;
        const uint32_t sl = (uint32_t)e >> th_log2, hl = (uint32_t)e & th_mask;
        f[j] = e < kTileRows ? factor[slot][(hl << p.ts_log2) + (sl & ts_mask)] : kNoRow;
        const int64_t ss = s0 + sl, hh = h0 + hl;
        off_in[j] = bb * p.oi_bs + ss * p.oi_rs + hh * p.oi_hs + dc * 16;
        off_out[j] = bb * p.o_bs + ss * p.o_rs + hh * p.o_hs + dc * 16;
        raw[j] = u32x4{0u, 0u, 0u, 0u};
        if (f[j] > 0.f) raw[j] = *reinterpret_cast<const u32x4*>(p.out_in + off_in[j]);   // (a factor of 0: the row is not fetched)
      }
#pragma unroll
      for (int j = 0; j < kInFlight; ++j) {
        if (f[j] < 0.f) continue;
        *reinterpret_cast<u32x4*>(p.out + off_out[j]) = f[j] == 1.f || f[j] == 0.f ? raw[j] : scale_chunk(raw[j], f[j], p.dt);
      }
    }
  }
}

// workgroup sum of one float per thread in a fixed order, valid in thread 0
__device__ __forceinline__ float block_sum(float x, float* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// grid: h * nblk workgroups; workgroup (head, i) -> ws[head * nblk + i]
__global__ void __launch_bounds__(kThreads) fa_sink_dsink_partial_kernel(const DsinkK p) {
  __shared__ float red4[4];
  const uint32_t blk = blockIdx.x % (uint32_t)p.nblk;
  const int64_t hh = blockIdx.x / (uint32_t)p.nblk;
  const float sv = load_sink(p.sink, hh * p.sink_st, p.sink_dt);
  const uint32_t step = (uint32_t)p.nblk * kThreads;
  float acc = 0.f;
  for (uint32_t r0 = blk * kThreads + threadIdx.x; r0 < p.rows; r0 += kInFlight * step) {
    float w[kInFlight], dd[kInFlight];
#pragma unroll
    for (int j = 0; j < kInFlight; ++j) {
      const uint32_t r = r0 + j * step;              // (< 2^31 + 4 * 64 * 256: no wrap)
      w[j] = 0.f;
      dd[j] = 0.f;
      if (r < p.rows) {
        const uint32_t bb = r / p.s, ss = r - bb * p.s;
        const float l = p.l[(int64_t)bb * p.l_bs + (int64_t)ss * p.l_rs + hh * p.l_hs];
        if (live(l)) w[j] = expf(sv - l);            // (lse' >= s: at most 1)
        if (w[j] != 0.f) dd[j] = p.d[(int64_t)bb * p.d_bs + (int64_t)ss * p.d_rs + hh * p.d_hs];   // (a skipped row's softmax_d is not fetched)
      }
    }
#pragma unroll
    for (int j = 0; j < kInFlight; ++j)
      if (w[j] != 0.f) acc = fmaf(w[j], dd[j], acc);
  }
  const float sum = block_sum(acc, red4);
  if (threadIdx.x == 0) p.ws[hh * p.nblk + blk] = sum;
}

// grid: h workgroups of one wave
__global__ void __launch_bounds__(64) fa_sink_dsink_finish_kernel(const DsinkK p) {
  const int64_t hh = blockIdx.x;
  float x = (int)threadIdx.x < p.nblk ? p.ws[hh * p.nblk + threadIdx.x] : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if (threadIdx.x == 0) p.dsink[hh * p.dsink_st] = -x;
}

}  // namespace fs

// ---------------------------------------------------------------- host side: validation and the launches ----------------------------------------------------------------
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

bool o_dtype(int dt) { return dt == FA_SINK_DTYPE_FP16 || dt == FA_SINK_DTYPE_BF16; }
int sink_size(int dt) { return dt == FA_SINK_DTYPE_FP32 ? 4 : o_dtype(dt) ? 2 : 0; }

// One stride of an out tensor, in 2-byte elements; a dimension of one element may have any stride.
int check_o_stride(const char* fn, const char* tensor, const char* what, int64_t stride, int64_t extent, bool output) {
  if (extent <= 1) return kOk;
  if ((stride * 2) % 16 != 0) return fail(kInvalid, "%s: %s: %s stride %lld (elements of 2 bytes) must be a multiple of 16 bytes", fn, tensor, what, (long long)stride);
  if (output && stride == 0) return fail(kInvalid, "%s: %s: %s stride of an output must not be 0", fn, tensor, what);
  return kOk;
}

int check_out_stride(const char* fn, const char* tensor, const char* what, int64_t stride, int64_t extent) {
  if (extent > 1 && stride == 0) return fail(kInvalid, "%s: %s: %s stride of an output must not be 0", fn, tensor, what);
  return kOk;
}

struct View {   // a three-dimensional strided tensor: byte range and identity
  const void* p;
  int64_t st[3];
  uintptr_t lo, hi;
};

View view_of(const void* p, int64_t bs, int64_t rs, int64_t hs, const int32_t (&n)[3], int64_t esz, int64_t last_bytes) {
  View v{p, {bs, rs, hs}, 0, 0};
  int64_t neg = 0, pos = 0;
  for (int i = 0; i < 3; ++i) {
    if (n[i] <= 1) {
      v.st[i] = 0;   // (never used: not part of the identity)
      continue;
    }
    const int64_t span = (int64_t)(n[i] - 1) * v.st[i] * esz;
    (span < 0 ? neg : pos) += span;
  }
  v.lo = (uintptr_t)p + neg;
  v.hi = (uintptr_t)p + pos + last_bytes;
  return v;
}

bool same_view(const View& a, const View& b) { return a.p == b.p && a.st[0] == b.st[0] && a.st[1] == b.st[1] && a.st[2] == b.st[2]; }
bool overlap(const View& a, const View& b) { return a.lo < b.hi && b.lo < a.hi; }

int check_sink(const char* fn, const void* sink, int dt) {
  if (!sink) return fail(kInvalid, "%s: sink must be non-NULL", fn);
  if (((uintptr_t)sink & (uintptr_t)(sink_size(dt) - 1)) != 0) return fail(kInvalid, "%s: sink must be %d-byte aligned", fn, sink_size(dt));
  return kOk;
}

int dsink_blocks(int64_t rows) { return (int)std::min<int64_t>(FA_SINK_DSINK_MAX_BLOCKS, (rows + fs::kDsinkRowsPerBlock - 1) / fs::kDsinkRowsPerBlock); }

int launched(const char* fn) {
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    g_kernel = "";
    return fail(kLaunch, "%s: launch failed: %s", fn, hipGetErrorString(e));
  }
  return kOk;
}

}  // namespace

extern "C" {

int fa_sink_abi_version(void) { return FA_SINK_ABI_VERSION; }
int fa_sink_sizeof_apply_params(void) { return (int)sizeof(FaSinkApplyParams); }
int fa_sink_sizeof_dsink_params(void) { return (int)sizeof(FaSinkDsinkParams); }
const char* fa_sink_last_error(void) { return g_err; }
const char* fa_sink_last_kernel_name(void) { return g_kernel; }

int fa_sink_apply(const FaSinkApplyParams* a, void* stream) {
  static const char* const kFn = "fa_sink_apply";
  g_kernel = "";
  if (!a) return fail(kInvalid, "%s: params is NULL", kFn);
  g_err[0] = 0;
  if (!o_dtype(a->dtype)) return fail(kInvalid, "%s: dtype must be fp16 (0) or bf16 (1)", kFn);
  if (!sink_size(a->sink_dtype)) return fail(kInvalid, "%s: sink_dtype must be fp16 (0), bf16 (1) or fp32 (3)", kFn);
  if (a->b < 0 || a->s < 0 || a->h < 0) return fail(kInvalid, "%s: b, s and h must not be negative", kFn);
  if (a->d < 8 || a->d > 512 || a->d % 8 != 0) return fail(kInvalid, "%s: d = %d: the head dimension must be a multiple of 8 in [8, 512]", kFn, a->d);
  if (a->b == 0 || a->s == 0 || a->h == 0) return kOk;
  if ((int64_t)a->b * a->s > INT32_MAX || (int64_t)a->b * a->s * a->h > INT32_MAX) return fail(kInvalid, "%s: b * s * h must be below 2^31", kFn);
  if (!a->out_in) return fail(kInvalid, "%s: out_in must be non-NULL", kFn);
  if (!a->lse_in) return fail(kInvalid, "%s: lse_in must be non-NULL", kFn);
  if (!a->out) return fail(kInvalid, "%s: out must be non-NULL", kFn);
  if (!a->lse) return fail(kInvalid, "%s: lse must be non-NULL", kFn);
  int rc;
  if ((rc = check_sink(kFn, a->sink, a->sink_dtype))) return rc;
  if (((uintptr_t)a->out_in & 15u) != 0) return fail(kInvalid, "%s: out_in must be 16-byte aligned", kFn);
  if (((uintptr_t)a->out & 15u) != 0) return fail(kInvalid, "%s: out must be 16-byte aligned", kFn);
  if (((uintptr_t)a->lse_in & 3u) != 0) return fail(kInvalid, "%s: lse_in must be 4-byte aligned", kFn);
  if (((uintptr_t)a->lse & 3u) != 0) return fail(kInvalid, "%s: lse must be 4-byte aligned", kFn);
  if (((uintptr_t)a->lse_bwd & 3u) != 0) return fail(kInvalid, "%s: lse_bwd must be 4-byte aligned", kFn);
  if ((rc = check_o_stride(kFn, "out_in", "batch", a->out_in_batch_stride, a->b, false)) || (rc = check_o_stride(kFn, "out_in", "row", a->out_in_row_stride, a->s, false)) ||
      (rc = check_o_stride(kFn, "out_in", "head", a->out_in_head_stride, a->h, false)) || (rc = check_o_stride(kFn, "out", "batch", a->out_batch_stride, a->b, true)) ||
      (rc = check_o_stride(kFn, "out", "row", a->out_row_stride, a->s, true)) || (rc = check_o_stride(kFn, "out", "head", a->out_head_stride, a->h, true)) ||
      (rc = check_out_stride(kFn, "lse", "batch", a->lse_batch_stride, a->b)) || (rc = check_out_stride(kFn, "lse", "row", a->lse_row_stride, a->s)) ||
      (rc = check_out_stride(kFn, "lse", "head", a->lse_head_stride, a->h)))
    return rc;
  if (a->lse_bwd && ((rc = check_out_stride(kFn, "lse_bwd", "batch", a->lse_bwd_batch_stride, a->b)) || (rc = check_out_stride(kFn, "lse_bwd", "row", a->lse_bwd_row_stride, a->s)) ||
                     (rc = check_out_stride(kFn, "lse_bwd", "head", a->lse_bwd_head_stride, a->h))))
    return rc;
  {   // an output is exactly its input, or their address ranges are apart
    const int32_t n[3] = {a->b, a->s, a->h};
    const View oi = view_of(a->out_in, a->out_in_batch_stride, a->out_in_row_stride, a->out_in_head_stride, n, 2, (int64_t)a->d * 2);
    const View o = view_of(a->out, a->out_batch_stride, a->out_row_stride, a->out_head_stride, n, 2, (int64_t)a->d * 2);
    const View li = view_of(a->lse_in, a->lse_in_batch_stride, a->lse_in_row_stride, a->lse_in_head_stride, n, 4, 4);
    const View l = view_of(a->lse, a->lse_batch_stride, a->lse_row_stride, a->lse_head_stride, n, 4, 4);
    if (overlap(o, oi) && !same_view(o, oi)) return fail(kInvalid, "%s: out overlaps out_in without being the same tensor (same pointer and strides)", kFn);
    if (overlap(l, li) && !same_view(l, li)) return fail(kInvalid, "%s: lse overlaps lse_in without being the same tensor (same pointer and strides)", kFn);
    if (overlap(o, li) || overlap(o, l) || overlap(l, oi)) return fail(kInvalid, "%s: out / out_in overlap lse / lse_in", kFn);
    if (a->lse_bwd) {
      const View lb = view_of(a->lse_bwd, a->lse_bwd_batch_stride, a->lse_bwd_row_stride, a->lse_bwd_head_stride, n, 4, 4);
      if (overlap(lb, l)) return fail(kInvalid, "%s: lse_bwd overlaps lse", kFn);
      if (overlap(lb, li) && !same_view(lb, li)) return fail(kInvalid, "%s: lse_bwd overlaps lse_in without being the same tensor (same pointer and strides)", kFn);
      if (overlap(lb, o) || overlap(lb, oi)) return fail(kInvalid, "%s: lse_bwd overlaps out / out_in", kFn);
    }
  }

  fs::ApplyK k{};
  k.out_in = (const char*)a->out_in; k.lse_in = a->lse_in; k.sink = (const char*)a->sink;
  k.out = (char*)a->out; k.lse = a->lse; k.lse_bwd = a->lse_bwd;
  k.oi_bs = a->out_in_batch_stride * 2; k.oi_rs = a->out_in_row_stride * 2; k.oi_hs = a->out_in_head_stride * 2;
  k.o_bs = a->out_batch_stride * 2; k.o_rs = a->out_row_stride * 2; k.o_hs = a->out_head_stride * 2;
  k.li_bs = a->lse_in_batch_stride; k.li_rs = a->lse_in_row_stride; k.li_hs = a->lse_in_head_stride;
  k.l_bs = a->lse_batch_stride; k.l_rs = a->lse_row_stride; k.l_hs = a->lse_head_stride;
  k.lb_bs = a->lse_bwd_batch_stride; k.lb_rs = a->lse_bwd_row_stride; k.lb_hs = a->lse_bwd_head_stride;
  k.sink_st = a->sink_stride;
  k.s = (uint32_t)a->s; k.h = (uint32_t)a->h;
  k.ts_log2 = 0;
  while (k.ts_log2 < 6 && (1 << k.ts_log2) < a->s) ++k.ts_log2;
  const int64_t ts = 1 << k.ts_log2, th = fs::kTileRows / ts;
  k.tiles_s = (uint32_t)((a->s + ts - 1) / ts);
  k.tiles_h = (uint32_t)((a->h + th - 1) / th);
  const int64_t tiles = (int64_t)a->b * k.tiles_s * k.tiles_h;   // (<= b * s * h: below 2^31)
  k.tiles = (uint32_t)tiles;
  k.lpr = a->d / 8;
  k.rpp = fs::kThreads / k.lpr;
  k.dt = a->dtype; k.sink_dt = a->sink_dtype;
  g_kernel = "fa_sink_apply_kernel";
  hipLaunchKernelGGL(fs::fa_sink_apply_kernel, dim3((unsigned)std::min<int64_t>(tiles, fs::kBlocksPerCU * fs::kCUs)), dim3(fs::kThreads), 0, (hipStream_t)stream, k);
  return launched(kFn);
}

size_t fa_sink_dsink_workspace_bytes(const FaSinkDsinkParams* a) {
  if (!a || a->b <= 0 || a->s <= 0 || a->h <= 0) return 0;
  return (size_t)a->h * dsink_blocks((int64_t)a->b * a->s) * sizeof(float);
}

int fa_sink_dsink(const FaSinkDsinkParams* a, void* stream) {
  static const char* const kFn = "fa_sink_dsink";
  g_kernel = "";
  if (!a) return fail(kInvalid, "%s: params is NULL", kFn);
  g_err[0] = 0;
  if (!sink_size(a->sink_dtype)) return fail(kInvalid, "%s: sink_dtype must be fp16 (0), bf16 (1) or fp32 (3)", kFn);
  if (a->b < 0 || a->s < 0 || a->h < 0) return fail(kInvalid, "%s: b, s and h must not be negative", kFn);
  if (a->h == 0) return kOk;
  if ((int64_t)a->b * a->s > INT32_MAX || (int64_t)a->b * a->s * a->h > INT32_MAX) return fail(kInvalid, "%s: b * s * h must be below 2^31", kFn);
  const int64_t rows = (int64_t)a->b * a->s;
  if (!a->dsink) return fail(kInvalid, "%s: dsink must be non-NULL", kFn);
  if (((uintptr_t)a->dsink & 3u) != 0) return fail(kInvalid, "%s: dsink must be 4-byte aligned", kFn);
  int rc;
  if ((rc = check_out_stride(kFn, "dsink", "head", a->dsink_stride, a->h))) return rc;
  fs::DsinkK k{};
  k.dsink = a->dsink; k.dsink_st = a->dsink_stride;
  if (rows > 0) {
    if (!a->softmax_d) return fail(kInvalid, "%s: softmax_d must be non-NULL", kFn);
    if (!a->lse_bwd) return fail(kInvalid, "%s: lse_bwd must be non-NULL", kFn);
    if ((rc = check_sink(kFn, a->sink, a->sink_dtype))) return rc;
    if (((uintptr_t)a->softmax_d & 3u) != 0) return fail(kInvalid, "%s: softmax_d must be 4-byte aligned", kFn);
    if (((uintptr_t)a->lse_bwd & 3u) != 0) return fail(kInvalid, "%s: lse_bwd must be 4-byte aligned", kFn);
    const size_t need = fa_sink_dsink_workspace_bytes(a);
    if (!a->workspace) return fail(kInvalid, "%s: workspace must be non-NULL", kFn);
    if (((uintptr_t)a->workspace & 3u) != 0) return fail(kInvalid, "%s: workspace must be 4-byte aligned", kFn);
    if (a->workspace_bytes < 0 || (uint64_t)a->workspace_bytes < need)
      return fail(kInvalid, "%s: workspace_bytes = %lld is too small: these shapes need %llu bytes (fa_sink_dsink_workspace_bytes)", kFn, (long long)a->workspace_bytes, (unsigned long long)need);
    k.d = a->softmax_d; k.l = a->lse_bwd; k.sink = (const char*)a->sink; k.ws = (float*)a->workspace;
    k.d_bs = a->softmax_d_batch_stride; k.d_rs = a->softmax_d_row_stride; k.d_hs = a->softmax_d_head_stride;
    k.l_bs = a->lse_bwd_batch_stride; k.l_rs = a->lse_bwd_row_stride; k.l_hs = a->lse_bwd_head_stride;
    k.sink_st = a->sink_stride;
    k.rows = (uint32_t)rows; k.s = (uint32_t)a->s;
    k.nblk = dsink_blocks(rows);
    k.sink_dt = a->sink_dtype;
    g_kernel = "fa_sink_dsink_partial_kernel";
    hipLaunchKernelGGL(fs::fa_sink_dsink_partial_kernel, dim3((unsigned)((int64_t)a->h * k.nblk)), dim3(fs::kThreads), 0, (hipStream_t)stream, k);
    if ((rc = launched(kFn))) return rc;
  } else {
    g_kernel = "fa_sink_dsink_finish_kernel";   // (no rows: dsink = 0, nothing but dsink is touched)
  }
  hipLaunchKernelGGL(fs::fa_sink_dsink_finish_kernel, dim3((unsigned)a->h), dim3(64), 0, (hipStream_t)stream, k);
  return launched(kFn);
}

}  // extern "C"
