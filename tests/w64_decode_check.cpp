// Host program of tests/test_w64_decode_cpu.py (compiled by the test with the host compiler): the multiply-shift reciprocals and the block decode of the
// 64-rows-per-wave forward (csrc/fa_kernel_params.h: fastdiv_make / fastdiv / fwd_w64_decode) are host-callable, so they are walked here, on the CPU.
//   w64_decode_check div                          every divisor class x numerator class against / (prints "ok <count>" or the first mismatch)
//   w64_decode_check walk b h h_k nmb wr grid     the persistent walk of a dense launch: one line "vb round b h m_block" per block (-1 -1 -1 = padding)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fa_kernel_params.h"
#include "fa_launch.h"

static long long checked = 0;
static bool check(int32_t n, int32_t d, fa::FastDiv f) {
  ++checked;
  if (fa::fastdiv(n, f) == n / d) return true;
  printf("MISMATCH n=%d d=%d got=%d want=%d\n", n, d, fa::fastdiv(n, f), n / d);
  return false;
}

// numerators of one divisor: the ends of the range, every multiple's neighbourhood at a spread of quotients, and a stride through the whole range
static bool check_divisor(int32_t d, int stride_points) {
  const fa::FastDiv f = fa::fastdiv_make(d);
  const int64_t top = 0x7fffffffll;
  for (int64_t n : {0ll, 1ll, 2ll, (long long)top - 1, (long long)top})
    if (!check((int32_t)n, d, f)) return false;
  const int64_t qmax = top / d;
  for (int i = 0; i <= 64; ++i) {
    const int64_t q = qmax * i / 64;
    for (int64_t n = q * d - 2; n <= q * d + 2; ++n)
      if (n >= 0 && n <= top && !check((int32_t)n, d, f)) return false;
  }
  const int64_t step = top / stride_points + 1;
  for (int64_t n = (int64_t)d % step; n <= top; n += step)
    if (!check((int32_t)n, d, f)) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "div")) {
    // every divisor a head count or a block count can be (<= 65535), exhaustively against small numerators as well
    for (int32_t d = 1; d <= 65535; ++d) {
      if (!check_divisor(d, 256)) return 1;
      const fa::FastDiv f = fa::fastdiv_make(d);
      if (d <= 1024) for (int32_t n = 0; n < 65536; ++n) if (!check(n, d, f)) return 1;
    }
    // unit sizes (heads per group x blocks) beyond that: powers of two and their neighbours, the largest values, a multiplicative sweep
    for (int s = 16; s <= 31; ++s)
      for (int64_t d = (1ll << s) - 2; d <= (1ll << s) + 2; ++d)
        if (d <= 0x7fffffffll && !check_divisor((int32_t)d, 4096)) return 1;
    for (int64_t d = 65536; d <= 0x7fffffffll; d = d * 1009 / 1000 + 1)
      if (!check_divisor((int32_t)d, 1024)) return 1;
    printf("ok %lld\n", checked);
    return 0;
  }
  if (argc == 8 && !strcmp(argv[1], "walk")) {
    fa::FwdK p;
    memset(&p, 0, sizeof(p));
    p.b = atoi(argv[2]); p.h = atoi(argv[3]); p.h_k = atoi(argv[4]); p.nmb = atoi(argv[5]); p.wr = atoi(argv[6]); p.wl = -1;
    const int grid = atoi(argv[7]);
    p.hk_ratio = p.h / p.h_k;
    fa::choose_units(p.b, p.h_k, p.hk_ratio, p.nmb, p.n_units, p.unit_size, p.unit_hpx);
    const long long total = fa::units_grid(p.n_units, p.unit_size);
    p.persist_total = (int)total;
    fa::fwd_w64_reciprocals(p);
    printf("units %d %d %d total %lld\n", p.n_units, p.unit_size, p.unit_hpx, total);
    // the kernel's `snake`: rounds made of whole units under a right bound
    const int g8 = grid >> 3;
    const bool snake = p.wr >= 0 && p.unit_size > 1 && g8 - fa::fastdiv(g8, fa::rc_get(p.rc, fa::RC_UNIT)) * p.unit_size == 0;
    for (int first = 0; first < grid; ++first)
      for (int vb = first, round = 0; vb < total; vb += grid, ++round) {
        int32_t b = -1, h = -1, mb = -1;
        if (!fa::fwd_w64_decode(p, p.rc, vb, snake && (round & 1), b, h, mb)) b = h = mb = -1;
        printf("%d %d %d %d %d\n", vb, round, b, h, mb);
      }
    return 0;
  }
  fprintf(stderr, "usage: %s div | walk b h h_k nmb wr grid\n", argv[0]);
  return 2;
}
