// libfa_gfx950_quant.so (include/fa_gfx950_quant.h): bf16 / fp16 -> OCP e4m3 with one fp32 descale per (batch entry, KV head), and the quantising append
// of the e4m3 KV cache.  HBM- and launch-bound: every lane moves 16-element chunks (two 16-byte loads, one 16-byte store), the maximum is taken on the
// bit patterns (|x| of a non-negative bf16 / fp16 orders as an unsigned integer) and crosses workgroups as ONE vector atomicMax per workgroup.
//
// The unit of work is a CHUNK: 16 consecutive channels of one head of one row.  A group (b, g) -- heads g*r .. g*r+r-1 of batch entry b, all its rows --
// is a list of rows * r * (d / 16) chunks, numbered row-major (row, head in group, chunk in head): consecutive lanes read consecutive memory wherever the
// tensor is dense.  A lane finds its first chunk with two divisions and walks on in steps of 256 chunks with carries (Walk below).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/fa_gfx950_quant.h"

namespace fq {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr int kChunksPerThread = 4;                       // FA_QUANT_ONE_LAUNCH_MAX_ELEMS = 256 * 4 * 16
constexpr int kTile = kThreads * kChunksPerThread;        // chunks a workgroup holds at a time
static_assert(kTile * 16 == FA_QUANT_ONE_LAUNCH_MAX_ELEMS, "the header states the one-launch bound");

struct Tensor {   // device view of one FaQuantTensor
  const uint16_t* x;
  uint8_t* y;
  float* ds;
  const int32_t* cu;
  int64_t x_bs, x_rs, x_hs, y_bs, y_rs, y_hs, ds_bs, ds_hs;
  int32_t r;          // heads per group
  int32_t rows;       // fixed-length: rows per entry
  int32_t is_static;
  int32_t ws_off;     // first scratch word of this tensor (dynamic, two-pass)
};

struct QuantK {
  Tensor t[FA_QUANT_MAX_TENSORS];
  uint32_t* ws;
  int32_t h_k, cpr;   // cpr = d / 16 chunks per head row
};

struct AppendK {
  const uint16_t* knew; const uint16_t* vnew; uint8_t* kcache; uint8_t* vcache; const float* kds; const float* vds;
  int64_t kn_bs, kn_rs, kn_hs, vn_bs, vn_rs, vn_hs, kc_bs, kc_rs, kc_hs, vc_bs, vc_rs, vc_hs, kds_bs, kds_hs, vds_bs, vds_hs;
  const int32_t* seqlens_k; const int32_t* kv_batch_idx; const int32_t* block_table;
  int64_t block_table_bs;
  int32_t page_size, b, s_new, h_k, cpr;
};

struct Walk { int row, hh, dc; };   // a chunk's place in its group: row, head within the group, chunk within the head

__device__ __forceinline__ Walk walk_at(int chunk, int cpr, int r) {
  const int hr = chunk / cpr;
  return {hr / r, hr % r, chunk % cpr};
}
__device__ __forceinline__ void walk_step(Walk& w, const Walk& s, int cpr, int r) {   // w += s, s = walk_at(step): every field carries at most once
  w.dc += s.dc;
  if (w.dc >= cpr) { w.dc -= cpr; ++w.hh; }
  w.hh += s.hh;
  if (w.hh >= r) { w.hh -= r; ++w.row; }
  w.row += s.row;
}

struct Group { const uint16_t* x; uint8_t* y; float* ds; int n_chunks; };

__device__ __forceinline__ Group group_of(const Tensor& t, int b, int g, int cpr) {
  const int row0 = t.cu ? t.cu[b] : 0;
  const int rows = t.cu ? t.cu[b + 1] - row0 : t.rows;
  Group gr;
  gr.x = t.x + (t.cu ? 0 : (int64_t)b * t.x_bs) + (int64_t)row0 * t.x_rs + (int64_t)g * t.r * t.x_hs;
  gr.y = t.y + (t.cu ? 0 : (int64_t)b * t.y_bs) + (int64_t)row0 * t.y_rs + (int64_t)g * t.r * t.y_hs;
  gr.ds = t.ds + (int64_t)b * t.ds_bs + (int64_t)g * t.ds_hs;
  gr.n_chunks = rows > 0 ? rows * t.r * cpr : 0;
  return gr;
}

// max |x| of two packed 16-bit floats per word, as bit patterns
__device__ __forceinline__ uint32_t pk_absmax(uint32_t m, u32x4 v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const u16x2 a = __builtin_bit_cast(u16x2, v[j] & 0x7fff7fffu);
    m = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, m), a));
  }
  return m;
}

// workgroup maximum of one 32-bit word per thread, returned to every thread
__device__ __forceinline__ uint32_t block_max(uint32_t m, uint32_t* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  return max(max(lds[0], lds[1]), max(lds[2], lds[3]));
}

template <bool BF16>
__device__ __forceinline__ float amax_of_bits(uint32_t bits) {   // the 15-bit pattern of the largest magnitude, exact in fp32
  if (BF16) return __builtin_bit_cast(float, bits << 16);
  return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
}

__device__ __forceinline__ float descale_of(float amax) { return amax > 0.f ? __fdiv_rn(amax, 448.0f) : 1.0f; }

template <bool BF16>
__device__ __forceinline__ void unpack2(uint32_t w, float& lo, float& hi) {
  if (BF16) {
    lo = __builtin_bit_cast(float, w << 16);
    hi = __builtin_bit_cast(float, w & 0xffff0000u);
  } else {
    lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu));
    hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
  }
}

// 16 elements (two 16-byte loads) -> 16 e4m3 bytes: y = e4m3_rne(clamp(x * inv, -448, 448)), v_cvt_pk_fp8_f32 (OCP e4m3, round to nearest even)
template <bool BF16>
__device__ __forceinline__ u32x4 cast16(u32x4 a, u32x4 b, float inv) {
  u32x4 out;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t w0 = j < 2 ? a[2 * j] : b[2 * j - 4], w1 = j < 2 ? a[2 * j + 1] : b[2 * j - 3];
    float e0, e1, e2, e3;
    unpack2<BF16>(w0, e0, e1);
    unpack2<BF16>(w1, e2, e3);
    e0 = __builtin_amdgcn_fmed3f(e0 * inv, -448.0f, 448.0f);
    e1 = __builtin_amdgcn_fmed3f(e1 * inv, -448.0f, 448.0f);
    e2 = __builtin_amdgcn_fmed3f(e2 * inv, -448.0f, 448.0f);
    e3 = __builtin_amdgcn_fmed3f(e3 * inv, -448.0f, 448.0f);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(e0, e1, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(e2, e3, w, true);
    out[j] = (uint32_t)w;
  }
  return out;
}

// One tile of a group: the chunks base + threadIdx.x + 256 k, k < 4, that exist.
struct Tile {
  u32x4 a[kChunksPerThread], b[kChunksPerThread];
  int64_t yoff[kChunksPerThread];
  bool ok[kChunksPerThread];
};

__device__ __forceinline__ void load_tile(Tile& tl, const Tensor& t, const Group& gr, int base, int cpr) {
  Walk w = walk_at(base + (int)threadIdx.x, cpr, t.r);
  const Walk step = walk_at(kThreads, cpr, t.r);
#pragma unroll
  for (int k = 0; k < kChunksPerThread; ++k) {
    tl.ok[k] = base + (int)threadIdx.x + k * kThreads < gr.n_chunks;
    tl.yoff[k] = (int64_t)w.row * t.y_rs + (int64_t)w.hh * t.y_hs + w.dc * 16;
    tl.a[k] = tl.b[k] = u32x4{0u, 0u, 0u, 0u};
    if (tl.ok[k]) {
      const u32x4* src = reinterpret_cast<const u32x4*>(gr.x + (int64_t)w.row * t.x_rs + (int64_t)w.hh * t.x_hs + w.dc * 16);
      tl.a[k] = src[0];
      tl.b[k] = src[1];
    }
    walk_step(w, step, cpr, t.r);
  }
}

template <bool BF16>
__device__ __forceinline__ void store_tile(const Tile& tl, const Group& gr, float inv) {
#pragma unroll
  for (int k = 0; k < kChunksPerThread; ++k)
    if (tl.ok[k]) *reinterpret_cast<u32x4*>(gr.y + tl.yoff[k]) = cast16<BF16>(tl.a[k], tl.b[k], inv);
}

__device__ __forceinline__ uint32_t tile_absmax(const Tile& tl, uint32_t m) {
#pragma unroll
  for (int k = 0; k < kChunksPerThread; ++k) m = pk_absmax(pk_absmax(m, tl.a[k]), tl.b[k]);   // (absent chunks are zeros)
  return m;
}

// The scratch clear of the two-pass path.  A kernel, not hipMemsetAsync: captured in a HIP graph, the runtime's memset node cleared the words on the first
// replay only and wrote a stale 16-byte pattern on every later one (measured with ROCm 7.2; tests/test_quant_fp8_gpu.py replays twice for this reason).
__global__ void __launch_bounds__(kThreads) fa_quant_clear_kernel(uint32_t* ws, int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) ws[i] = 0u;
}

// grid (workgroups per group, b * h_k, tensors).  Pass 1 of the two-pass path: the group's largest magnitude into its scratch word.
__global__ void __launch_bounds__(kThreads) fa_quant_amax_kernel(const QuantK p) {
  __shared__ uint32_t lds[4];
  const Tensor& t = p.t[blockIdx.z];
  if (t.is_static) return;
  const int b = blockIdx.y / p.h_k, g = blockIdx.y % p.h_k;
  const Group gr = group_of(t, b, g, p.cpr);
  uint32_t m = 0;
  for (int64_t base = (int64_t)blockIdx.x * kTile; base < gr.n_chunks; base += (int64_t)gridDim.x * kTile) {
    Tile tl;
    load_tile(tl, t, gr, (int)base, p.cpr);
    m = tile_absmax(tl, m);
  }
  m = max(m & 0xffffu, m >> 16);
  m = block_max(m, lds);
  if (threadIdx.x == 0 && m != 0) atomicMax(p.ws + t.ws_off + blockIdx.y, m);   // (the scratch starts at 0: nothing to add for an all-zero share)
}

// Pass 2: descale and inv once per workgroup, then the cast.  The workgroup 0 of a group writes a dynamic descale -- the only place that does.
template <bool BF16>
__global__ void __launch_bounds__(kThreads) fa_quant_cast_kernel(const QuantK p) {
  const Tensor& t = p.t[blockIdx.z];
  const int b = blockIdx.y / p.h_k, g = blockIdx.y % p.h_k;
  const Group gr = group_of(t, b, g, p.cpr);
  float ds;
  if (t.is_static) {
    ds = *gr.ds;
  } else {
    ds = descale_of(amax_of_bits<BF16>(p.ws[t.ws_off + blockIdx.y]));
    if (blockIdx.x == 0 && threadIdx.x == 0) *gr.ds = ds;
  }
  const float inv = __fdiv_rn(1.0f, ds);
  for (int64_t base = (int64_t)blockIdx.x * kTile; base < gr.n_chunks; base += (int64_t)gridDim.x * kTile) {
    Tile tl;
    load_tile(tl, t, gr, (int)base, p.cpr);
    store_tile<BF16>(tl, gr, inv);
  }
}

// One-launch path: grid (1, b * h_k, tensors); the workgroup owns the group and keeps it in registers between the maximum and the cast.
template <bool BF16>
__global__ void __launch_bounds__(kThreads) fa_quant_fused_kernel(const QuantK p) {
  __shared__ uint32_t lds[4];
  const Tensor& t = p.t[blockIdx.z];
  const int b = blockIdx.y / p.h_k, g = blockIdx.y % p.h_k;
  const Group gr = group_of(t, b, g, p.cpr);
  Tile tl;
  load_tile(tl, t, gr, 0, p.cpr);
  float ds;
  if (t.is_static) {
    ds = *gr.ds;
  } else {
    uint32_t m = tile_absmax(tl, 0);
    m = block_max(max(m & 0xffffu, m >> 16), lds);
    ds = descale_of(amax_of_bits<BF16>(m));
    if (threadIdx.x == 0) *gr.ds = ds;
  }
  store_tile<BF16>(tl, gr, __fdiv_rn(1.0f, ds));
}

// Quantising append: grid (chunks of one entry's new rows / 256, b); one thread moves one chunk of a key row and the matching chunk of the value row.
template <bool BF16>
__global__ void __launch_bounds__(kThreads) fa_quant_append_kernel(const AppendK p) {
  const int per_b = p.s_new * p.h_k * p.cpr;
  const int b = blockIdx.y;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < per_b; i += gridDim.x * kThreads) {
    const int c = i % p.cpr, hk = (i / p.cpr) % p.h_k, s = i / (p.cpr * p.h_k);
    const int row = (p.seqlens_k ? p.seqlens_k[b] : 0) + s;
    int64_t koff, voff;
    if (p.block_table) {
      const int page = row / p.page_size;
      const int blk = p.block_table[(int64_t)b * p.block_table_bs + page];
      koff = (int64_t)blk * p.kc_bs + (int64_t)(row - page * p.page_size) * p.kc_rs;
      voff = (int64_t)blk * p.vc_bs + (int64_t)(row - page * p.page_size) * p.vc_rs;
    } else {
      const int bkv = p.kv_batch_idx ? p.kv_batch_idx[b] : b;
      koff = (int64_t)bkv * p.kc_bs + (int64_t)row * p.kc_rs;
      voff = (int64_t)bkv * p.vc_bs + (int64_t)row * p.vc_rs;
    }
    const u32x4* ks = reinterpret_cast<const u32x4*>(p.knew + (int64_t)b * p.kn_bs + (int64_t)s * p.kn_rs + (int64_t)hk * p.kn_hs + c * 16);
    const u32x4* vs = reinterpret_cast<const u32x4*>(p.vnew + (int64_t)b * p.vn_bs + (int64_t)s * p.vn_rs + (int64_t)hk * p.vn_hs + c * 16);
    const u32x4 k0 = ks[0], k1 = ks[1], v0 = vs[0], v1 = vs[1];
    const float kinv = __fdiv_rn(1.0f, p.kds[(int64_t)b * p.kds_bs + (int64_t)hk * p.kds_hs]);
    const float vinv = __fdiv_rn(1.0f, p.vds[(int64_t)b * p.vds_bs + (int64_t)hk * p.vds_hs]);
    *reinterpret_cast<u32x4*>(p.kcache + koff + (int64_t)hk * p.kc_hs + c * 16) = cast16<BF16>(k0, k1, kinv);
    *reinterpret_cast<u32x4*>(p.vcache + voff + (int64_t)hk * p.vc_hs + c * 16) = cast16<BF16>(v0, v1, vinv);
  }
}

}  // namespace fq

// ---------------------------------------------------------------- host side: validation and launches ----------------------------------------------------------------
namespace {

enum { kOk = 0, kInvalid = -1, kUnsupported = -2, kLaunch = -3, kWorkspace = -4 };   // FA_OK / FA_ERR_* of include/fa_gfx950.h
enum { kFp16 = 0, kBf16 = 1 };

thread_local char g_err[512] = {0};

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

const char* const kSlot[FA_QUANT_MAX_TENSORS] = {"tensor 0", "tensor 1", "tensor 2"};

// One stride of a tensor: `unit` elements (inputs: 8) or bytes (outputs: 16); a dimension of one element may have any stride.
int check_stride(const char* fn, const char* slot, const char* what, int64_t stride, int64_t extent, int unit, bool output) {
  if (extent <= 1) return kOk;
  if (stride % unit != 0)
    return fail(kInvalid, "%s: %s: %s stride %lld must be a multiple of %d %s", fn, slot, what, (long long)stride, unit, output ? "bytes" : "elements");
  if (output && stride == 0) return fail(kInvalid, "%s: %s: %s stride of an output must not be 0", fn, slot, what);
  return kOk;
}

struct Plan { bool one_launch; bool any_dynamic; int64_t max_chunks; int64_t ws_words; };

// Everything fa_quant_e4m3 refuses, except the workspace (fa_quant_workspace_bytes runs this too).
int validate(const char* fn, const FaQuantParams* a, Plan& pl) {
  if (!a) return fail(kInvalid, "%s: params is NULL", fn);
  g_err[0] = 0;
  if (a->n_tensors < 1 || a->n_tensors > FA_QUANT_MAX_TENSORS) return fail(kInvalid, "%s: n_tensors = %d: one call takes 1 to %d tensors", fn, a->n_tensors, FA_QUANT_MAX_TENSORS);
  if (a->dtype != kFp16 && a->dtype != kBf16) return fail(kInvalid, "%s: the inputs must be fp16 or bf16", fn);
  if (a->b <= 0 || a->h_k <= 0 || (int64_t)a->b * a->h_k > 65535) return fail(kInvalid, "%s: b and h_k must be positive with b * h_k <= 65535", fn);
  if (a->d <= 0 || a->d % 16 != 0) return fail(kInvalid, "%s: the head dimension must be a multiple of 16 (got %d)", fn, a->d);
  if (a->path < FA_QUANT_PATH_AUTO || a->path > FA_QUANT_PATH_ONE_LAUNCH) return fail(kInvalid, "%s: path must be 0 (automatic), 1 (two-pass) or 2 (one launch)", fn);
  const int cpr = a->d / 16;
  bool fits = true;
  pl.any_dynamic = false;
  pl.max_chunks = 0;
  pl.ws_words = 0;
  for (int i = 0; i < a->n_tensors; ++i) {
    const FaQuantTensor& t = a->t[i];
    const char* s = kSlot[i];
    if (!t.x || !t.y || !t.descale) return fail(kInvalid, "%s: %s: x, y and descale must be non-NULL", fn, s);
    if (t.heads <= 0 || t.heads % a->h_k != 0) return fail(kInvalid, "%s: %s: heads (%d) must be a positive multiple of h_k (%d)", fn, s, t.heads, a->h_k);
    if (t.rows < 0) return fail(kInvalid, "%s: %s: rows must not be negative", fn, s);
    if (((uintptr_t)t.x & 15u) != 0) return fail(kInvalid, "%s: %s: x must be 16-byte aligned", fn, s);
    if (((uintptr_t)t.y & 15u) != 0) return fail(kInvalid, "%s: %s: y must be 16-byte aligned", fn, s);
    if (((uintptr_t)t.descale & 3u) != 0) return fail(kInvalid, "%s: %s: descale must be 4-byte aligned", fn, s);
    const bool packed = t.cu_seqlens != nullptr;
    const int64_t nb = packed ? 1 : a->b;   // (a packed tensor has no batch dimension)
    int rc;
    if ((rc = check_stride(fn, s, "x batch", t.x_batch_stride, nb, 8, false)) || (rc = check_stride(fn, s, "x row", t.x_row_stride, packed ? 2 : t.rows, 8, false)) ||
        (rc = check_stride(fn, s, "x head", t.x_head_stride, t.heads, 8, false)) || (rc = check_stride(fn, s, "y batch", t.y_batch_stride, nb, 16, true)) ||
        (rc = check_stride(fn, s, "y row", t.y_row_stride, packed ? 2 : t.rows, 16, true)) || (rc = check_stride(fn, s, "y head", t.y_head_stride, t.heads, 16, true)))
      return rc;
    if (!t.is_static && ((rc = check_stride(fn, s, "descale batch", t.descale_batch_stride, a->b, 1, true)) || (rc = check_stride(fn, s, "descale head", t.descale_head_stride, a->h_k, 1, true))))
      return rc;
    const int64_t chunks = (int64_t)t.rows * (t.heads / a->h_k) * cpr;   // of the largest possible group (packed: one entry owning every row)
    if (chunks > (1ll << 30)) return fail(kInvalid, "%s: %s: a group of more than 2^30 16-element chunks is not supported", fn, s);
    if (packed || chunks * 16 > FA_QUANT_ONE_LAUNCH_MAX_ELEMS) {
      fits = false;
      if (a->path == FA_QUANT_PATH_ONE_LAUNCH)
        return packed ? fail(kInvalid, "%s: %s: a packed tensor always takes the two-pass path (path = 2 refused)", fn, s)
                      : fail(kInvalid, "%s: %s: a group of %lld elements exceeds the one-launch bound of %d (path = 2 refused)", fn, s, (long long)(chunks * 16), FA_QUANT_ONE_LAUNCH_MAX_ELEMS);
    }
    pl.max_chunks = std::max(pl.max_chunks, chunks);
    if (!t.is_static) { pl.any_dynamic = true; pl.ws_words += (int64_t)a->b * a->h_k; }
  }
  pl.one_launch = a->path == FA_QUANT_PATH_ONE_LAUNCH || (a->path == FA_QUANT_PATH_AUTO && fits);
  if (pl.one_launch) pl.ws_words = 0;
  return kOk;
}

}  // namespace

extern "C" {

int fa_quant_abi_version(void) { return FA_QUANT_ABI_VERSION; }
int fa_sizeof_quant_tensor(void) { return (int)sizeof(FaQuantTensor); }
int fa_sizeof_quant_params(void) { return (int)sizeof(FaQuantParams); }
int fa_sizeof_quant_append_params(void) { return (int)sizeof(FaQuantAppendParams); }
const char* fa_quant_last_error(void) { return g_err; }

int64_t fa_quant_workspace_bytes(const FaQuantParams* a) {
  Plan pl;
  if (validate("fa_quant_workspace_bytes", a, pl) != kOk) return 0;
  return pl.ws_words * 4;
}

int fa_quant_e4m3(const FaQuantParams* a, void* stream) {
  const char* fn = "fa_quant_e4m3";
  Plan pl;
  if (int rc = validate(fn, a, pl)) return rc;
  if (pl.ws_words > 0) {
    if (!a->workspace || a->workspace_bytes < pl.ws_words * 4)
      return fail(kWorkspace, "%s: workspace missing or too small: the two-pass path needs %lld bytes (fa_quant_workspace_bytes)", fn, (long long)(pl.ws_words * 4));
    if (((uintptr_t)a->workspace & 3u) != 0) return fail(kInvalid, "%s: workspace must be 4-byte aligned", fn);
  }
  fq::QuantK k{};
  k.ws = (uint32_t*)a->workspace;
  k.h_k = a->h_k;
  k.cpr = a->d / 16;
  int32_t ws_off = 0;
  for (int i = 0; i < a->n_tensors; ++i) {
    const FaQuantTensor& t = a->t[i];
    fq::Tensor& d = k.t[i];
    d.x = (const uint16_t*)t.x; d.y = (uint8_t*)t.y; d.ds = t.descale; d.cu = t.cu_seqlens;
    d.x_bs = t.x_batch_stride; d.x_rs = t.x_row_stride; d.x_hs = t.x_head_stride;
    d.y_bs = t.y_batch_stride; d.y_rs = t.y_row_stride; d.y_hs = t.y_head_stride;
    d.ds_bs = t.descale_batch_stride; d.ds_hs = t.descale_head_stride;
    d.r = t.heads / a->h_k; d.rows = t.rows; d.is_static = t.is_static ? 1 : 0;
    d.ws_off = ws_off;
    if (!d.is_static && !pl.one_launch) ws_off += a->b * a->h_k;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool bf16 = a->dtype == kBf16;
  const unsigned groups = (unsigned)(a->b * a->h_k), nt = (unsigned)a->n_tensors;
  if (pl.one_launch) {
    if (bf16) hipLaunchKernelGGL(fq::fa_quant_fused_kernel<true>, dim3(1, groups, nt), dim3(fq::kThreads), 0, st, k);
    else hipLaunchKernelGGL(fq::fa_quant_fused_kernel<false>, dim3(1, groups, nt), dim3(fq::kThreads), 0, st, k);
  } else {
    // enough workgroups per group to fill the chip several times over when the groups are few; each walks its share of the tiles
    const int64_t tiles = std::max<int64_t>(1, (pl.max_chunks + fq::kTile - 1) / fq::kTile);
    const unsigned gx = (unsigned)std::min<int64_t>(tiles, std::max<int64_t>(1, (4096 + groups - 1) / groups));
    if (pl.any_dynamic) {
      hipLaunchKernelGGL(fq::fa_quant_clear_kernel, dim3((unsigned)((pl.ws_words + fq::kThreads - 1) / fq::kThreads)), dim3(fq::kThreads), 0, st, k.ws, (int)pl.ws_words);
      hipLaunchKernelGGL(fq::fa_quant_amax_kernel, dim3(gx, groups, nt), dim3(fq::kThreads), 0, st, k);
    }
    if (bf16) hipLaunchKernelGGL(fq::fa_quant_cast_kernel<true>, dim3(gx, groups, nt), dim3(fq::kThreads), 0, st, k);
    else hipLaunchKernelGGL(fq::fa_quant_cast_kernel<false>, dim3(gx, groups, nt), dim3(fq::kThreads), 0, st, k);
  }
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail(kLaunch, "%s: launch failed: %s", fn, hipGetErrorString(e));
  return kOk;
}

int fa_quant_kvcache_append(const FaQuantAppendParams* a, void* stream) {
  const char* fn = "fa_quant_kvcache_append";
  if (!a) return fail(kInvalid, "%s: params is NULL", fn);
  g_err[0] = 0;
  if (!a->knew || !a->vnew || !a->kcache || !a->vcache || !a->k_descale || !a->v_descale)
    return fail(kInvalid, "%s: knew, vnew, kcache, vcache, k_descale and v_descale must be non-NULL", fn);
  if (a->dtype != kFp16 && a->dtype != kBf16) return fail(kInvalid, "%s: knew / vnew must be fp16 or bf16", fn);
  if (a->d <= 0 || a->d % 16 != 0) return fail(kInvalid, "%s: the head dimension of an e4m3 cache must be a multiple of 16 (got %d)", fn, a->d);
  if (a->b < 0 || a->b > 65535 || a->seqlen_new < 0 || a->h_k <= 0) return fail(kInvalid, "%s: b must be in [0, 65535], seqlen_new >= 0 and h_k positive", fn);
  if (a->block_table && (a->page_block_size <= 0 || a->page_block_size % 256 != 0)) return fail(kInvalid, "%s: Paged KV cache block size must be divisible by 256", fn);
  if (a->block_table && a->cache_batch_idx) return fail(kInvalid, "%s: Paged KVcache does not support cache_batch_idx", fn);
  if ((int64_t)a->seqlen_new * a->h_k * (a->d / 16) > (1ll << 30)) return fail(kInvalid, "%s: more than 2^30 16-element chunks per batch entry are not supported", fn);
  if ((((uintptr_t)a->knew | (uintptr_t)a->vnew | (uintptr_t)a->kcache | (uintptr_t)a->vcache) & 15u) != 0)
    return fail(kInvalid, "%s: knew, vnew, kcache and vcache must be 16-byte aligned", fn);
  const int64_t many = 2;   // extents that are not parameters (cache entries, pages, cache rows) count as more than one
  int rc;
  if ((rc = check_stride(fn, "knew", "batch", a->knew_batch_stride, a->b, 8, false)) || (rc = check_stride(fn, "knew", "row", a->knew_row_stride, a->seqlen_new, 8, false)) ||
      (rc = check_stride(fn, "knew", "head", a->knew_head_stride, a->h_k, 8, false)) || (rc = check_stride(fn, "vnew", "batch", a->vnew_batch_stride, a->b, 8, false)) ||
      (rc = check_stride(fn, "vnew", "row", a->vnew_row_stride, a->seqlen_new, 8, false)) || (rc = check_stride(fn, "vnew", "head", a->vnew_head_stride, a->h_k, 8, false)) ||
      (rc = check_stride(fn, "kcache", "batch", a->kcache_batch_stride, many, 16, true)) || (rc = check_stride(fn, "kcache", "row", a->kcache_row_stride, many, 16, true)) ||
      (rc = check_stride(fn, "kcache", "head", a->kcache_head_stride, a->h_k, 16, true)) || (rc = check_stride(fn, "vcache", "batch", a->vcache_batch_stride, many, 16, true)) ||
      (rc = check_stride(fn, "vcache", "row", a->vcache_row_stride, many, 16, true)) || (rc = check_stride(fn, "vcache", "head", a->vcache_head_stride, a->h_k, 16, true)))
    return rc;
  if (a->b == 0 || a->seqlen_new == 0) return kOk;
  fq::AppendK k{};
  k.knew = (const uint16_t*)a->knew; k.vnew = (const uint16_t*)a->vnew; k.kcache = (uint8_t*)a->kcache; k.vcache = (uint8_t*)a->vcache;
  k.kds = a->k_descale; k.vds = a->v_descale;
  k.kn_bs = a->knew_batch_stride; k.kn_rs = a->knew_row_stride; k.kn_hs = a->knew_head_stride;
  k.vn_bs = a->vnew_batch_stride; k.vn_rs = a->vnew_row_stride; k.vn_hs = a->vnew_head_stride;
  k.kc_bs = a->kcache_batch_stride; k.kc_rs = a->kcache_row_stride; k.kc_hs = a->kcache_head_stride;
  k.vc_bs = a->vcache_batch_stride; k.vc_rs = a->vcache_row_stride; k.vc_hs = a->vcache_head_stride;
  k.kds_bs = a->k_descale_batch_stride; k.kds_hs = a->k_descale_head_stride; k.vds_bs = a->v_descale_batch_stride; k.vds_hs = a->v_descale_head_stride;
  k.seqlens_k = a->seqlens_k; k.kv_batch_idx = a->cache_batch_idx; k.block_table = a->block_table;
  k.block_table_bs = a->block_table_batch_stride; k.page_size = a->page_block_size;
  k.b = a->b; k.s_new = a->seqlen_new; k.h_k = a->h_k; k.cpr = a->d / 16;
  const int per_b = k.s_new * k.h_k * k.cpr;
  const dim3 grid((unsigned)std::min(1024, (per_b + fq::kThreads - 1) / fq::kThreads), (unsigned)a->b);
  if (a->dtype == kBf16) hipLaunchKernelGGL(fq::fa_quant_append_kernel<true>, grid, dim3(fq::kThreads), 0, (hipStream_t)stream, k);
  else hipLaunchKernelGGL(fq::fa_quant_append_kernel<false>, grid, dim3(fq::kThreads), 0, (hipStream_t)stream, k);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail(kLaunch, "%s: launch failed: %s", fn, hipGetErrorString(e));
  return kOk;
}

}  // extern "C"
