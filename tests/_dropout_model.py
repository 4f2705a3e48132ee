"""Host model of the dropout random stream (test infrastructure only; a plain helper, not a conftest).

Written from the text of DESIGN.md section 3.3 and the comments of csrc/fa_device.h -- nothing here is taken from a kernel's output:

  the random byte of element (batch b, query head h, query row i, key j) is byte (j & 3) of word 0 of Philox2x32-7 with counter (j >> 2, i) under the
  32-bit key K(seed, offset) ^ (b * H + h) * 0x9E3779B1; the element is kept iff byte <= threshold(p), and kept elements are scaled by 1 / (1 - p).

  K(seed, offset) = hash32(hash32(hash32(hash32(lo(seed) ^ 0x9E3779B9) ^ hi(seed)) ^ lo(offset)) ^ hi(offset)),
  hash32(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (mod 2^32)
  Philox2x32 round (seven of them): (c0, c1) <- (hi32(M * c0) ^ key ^ c1, lo32(M * c0)), key += 0x9E3779B9, M = 0xD256D193 (Random123)

  threshold(p) = floor((1.0f - p) * 255.0f) in SINGLE precision, as csrc/fa_api.cpp fill_dropout forms it from the C ABI's float p_dropout.  Python's
  double-precision math.floor(255.0 * (1.0 - p)) differs from it at p = 0.6 (101 against 102) and nowhere else over p = k/100, k/256, k/1000.

Packed batches (fa_varlen_fwd / fa_varlen_bwd): rows and keys count from 0 in each sequence and b is the sequence's index in cu_seqlens.  The kernels say so:

  csrc/fa_fwd.hip       "if (p.cu_q) {  // varlen: rows cu[b] .. cu[b+1]-1 ... sq = p.cu_q[b + 1] - c0; q_row0 = c0;"   (q_row0 only enters addresses)
                        "const int m0 = m_block * BM;" ... "const int my_row = w_row0 + qi;"                            (the row within the sequence)
                        "const uint32_t drop_key = drop ? drop_bh_key(p.rng, b * p.h + h) : 0u;"
                        "const int key0 = kv0 + 32 * kb + 8 * g4 + 4 * hi;" "const uint32_t bytes = drop_bytes(drop_key, my_row, key0 >> 2);"
                        (kv0 counts from the sequence's first key: K is addressed as "kp = (const E*)p.k + k_boff + k_row0 * p.k_rs + ...")
  csrc/fa_bwd.hip       dK/dV: "const uint32_t drop_key = drop ? drop_bh_key(p.rng, b * p.h + item_head(it)) : 0u;"
                               "hq = drop_bytes(drop_key, q0 + 8 * g + 4 * hi + (ki & 3), my_key >> 2);"  with q0 = item_m0(it) + 32 * qb
                        dQ:    "if (p.cu_q) { const int c0 = p.cu_q[b]; sq = p.cu_q[b + 1] - c0; q_row0 = c0; ..." "const int my_row = w_row0 + qi;"
                               "const uint32_t bytes = drop_bytes(drop_key, my_row, key0 >> 2);"
  csrc/fa_fwd_w64.hip, csrc/fa_bwd_w64.hip   "drop_bh_key(p.rng, b * p.h + h)", "drop_row[qb] = (unsigned)(w_row0 + 32 * qb + qi);"   (w_row0 within the sequence)
  csrc/fa_device.h      work_list_item(): "const int2 e = list[1 + item];" "b = e.x;" "blk = e.y;" -- a work-list entry carries the sequence's index and its block
                        within the sequence, so a launch that walks a list draws the same bytes as the dense grid.

Two implementations: numpy on uint32 / uint64 arrays (what the probes use), and the same three functions on Python ints with explicit masks
(tests/test_dropout_probe_cpu.py holds the one against the other: a guard of numpy's wrap-around and promotion rules, not of the kernels)."""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M = 0xD256D193
PHILOX_W = 0x9E3779B9
BH_ODD = 0x9E3779B1
ROUNDS = 7


# ---------------------------------------------------------------- numpy ----------------------------------------------------------------
def _u32(x):
    return (np.asarray(x).astype(np.uint64) & np.uint64(M32)).astype(np.uint64)   # kept in uint64 lanes, value < 2^32: products cannot wrap silently


def hash32(x):
    """uint64 array holding 32-bit values -> the same."""
    m = np.uint64(M32)
    x = _u32(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    x = x ^ (x >> np.uint64(16))
    return x


def _words(x):
    """a 64-bit quantity given as Python int(s) or an array of them -> (low word, high word) as uint64 arrays."""
    a = np.asarray(x, dtype=object)
    lo = np.vectorize(lambda t: int(t) & M32, otypes=[np.uint64])(a)
    hi = np.vectorize(lambda t: (int(t) >> 32) & M32, otypes=[np.uint64])(a)
    return lo, hi


def bh_key(seed, offset, bh):
    """The 32-bit stream key of (batch, query head) number bh = b * H + h; seed / offset are 64-bit (Python ints: a negative int64 counts as its two's complement)."""
    s_lo, s_hi = _words(seed)
    o_lo, o_hi = _words(offset)
    k = hash32(s_lo ^ np.uint64(PHILOX_W))
    k = hash32(k ^ s_hi)
    k = hash32(k ^ o_lo)
    k = hash32(k ^ o_hi)
    return k ^ ((_u32(bh) * np.uint64(BH_ODD)) & np.uint64(M32))


def drop_bytes(key, i, g):
    """Word 0 of Philox2x32-7 with counter (g, i) under `key`: the four random bytes of keys 4g .. 4g+3 of query row i (byte c <-> key 4g + c)."""
    m = np.uint64(M32)
    c0, c1, key = np.broadcast_arrays(_u32(g), _u32(i), _u32(key))
    for _ in range(ROUNDS):
        prod = c0 * np.uint64(PHILOX_M)                 # < 2^64: exact in uint64
        hi, lo = prod >> np.uint64(32), prod & m
        c0, c1 = hi ^ key ^ c1, lo
        key = (key + np.uint64(PHILOX_W)) & m
    return c0


def pair_byte(key, i, j):
    """The random byte of (row i, key j) under a stream key."""
    j = np.asarray(j).astype(np.uint64)
    return ((drop_bytes(key, i, j >> np.uint64(2)) >> (np.uint64(8) * (j & np.uint64(3)))) & np.uint64(0xFF)).astype(np.uint8)


def rand_bytes(seed, offset, B, H, Sq, Sk, b0=0):
    """uint8 (B, H, Sq, Sk): the byte of every pair of a fixed-length batch (b0: the index of the first entry -- one sequence of a packed batch is
    rand_bytes(seed, offset, 1, H, sq_b, sk_b, b0=b)[0])."""
    bh = (b0 + np.arange(B, dtype=np.uint64))[:, None] * np.uint64(H) + np.arange(H, dtype=np.uint64)[None, :]
    key = bh_key(seed, offset, bh)[:, :, None, None]
    i = np.arange(Sq, dtype=np.uint64)[None, None, :, None]
    g = np.arange((Sk + 3) // 4, dtype=np.uint64)[None, None, None, :]
    words = drop_bytes(key, i, g)                                           # one Philox call per four keys, as in the kernels
    byts = (words[..., None] >> (np.uint64(8) * np.arange(4, dtype=np.uint64))) & np.uint64(0xFF)
    return np.ascontiguousarray(byts.reshape(B, H, Sq, 4 * ((Sk + 3) // 4))[..., :Sk].astype(np.uint8))


def threshold(p):
    """floor((1.0f - p) * 255.0f), every step in single precision (csrc/fa_api.cpp fill_dropout)."""
    p_keep = np.float32(1.0) - np.float32(p)
    return int(np.floor(np.float32(p_keep * np.float32(255.0))))


def p_keep(p):
    """1.0f - p as the library holds it (a Python float)."""
    return float(np.float32(1.0) - np.float32(p))


def keep(seed, offset, p, B, H, Sq, Sk, b0=0):
    return rand_bytes(seed, offset, B, H, Sq, Sk, b0) <= threshold(p)


def keep_packed(seed, offset, p, H, lens_q, lens_k):
    """[bool (H, sq_b, sk_b)] per sequence of a packed batch: rows and keys count from 0 in each sequence, b is the sequence's index."""
    return [keep(seed, offset, p, 1, H, nq, nk, b0=b)[0] for b, (nq, nk) in enumerate(zip(lens_q, lens_k))]


# ---------------------------------------------------------------- the same on Python ints ----------------------------------------------------------------
def hash32_int(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def bh_key_int(seed, offset, bh):
    seed &= (1 << 64) - 1
    offset &= (1 << 64) - 1
    k = hash32_int((seed & M32) ^ PHILOX_W)
    k = hash32_int(k ^ (seed >> 32))
    k = hash32_int(k ^ (offset & M32))
    k = hash32_int(k ^ (offset >> 32))
    return k ^ (((bh & M32) * BH_ODD) & M32)


def drop_bytes_int(key, i, g):
    c0, c1, key = g & M32, i & M32, key & M32
    for _ in range(ROUNDS):
        prod = PHILOX_M * c0
        c0, c1 = ((prod >> 32) ^ key ^ c1) & M32, prod & M32
        key = (key + PHILOX_W) & M32
    return c0
