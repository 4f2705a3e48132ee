"""The block decode of the 64-rows-per-wave forward divides by launch constants through multiply-shift reciprocals (csrc/fa_kernel_params.h: fastdiv_make, fastdiv,
fwd_w64_decode -- host-callable on purpose).  tests/w64_decode_check.cpp, compiled here with the host compiler, walks them on the CPU:
  * fastdiv(n, d) == n // d for every divisor a head or block count can be (1 .. 65535; h and nmb are 16-bit, persist_total fits an int, so numerators stay below
    2^31) and for unit sizes up to 2^31 - 1 (powers of two, their neighbours, a multiplicative sweep); numerators: both ends of the range, the neighbourhood of
    multiples at 65 quotients from 0 to the largest, a stride through the whole range, and 0 .. 65535 exhaustively for the divisors up to 1024;
  * the (batch, head, query block) sequence of a persistent walk equals the mapping written with // and % in THIS file (choose_units of csrc/fa_launch.h,
    xcd_interleave of csrc/fa_device.h and the mirrored odd rounds as the kernel had them before round 7 -- restated here, independent of fastdiv), and visits
    every block exactly once.  tests/test_w64_walk_model_cpu.py models the key walk INSIDE a block and has no block decode to reuse: only its block height BM is
    imported, so that the number of query blocks is formed as that model forms it."""
import os
import shutil
import subprocess

import pytest

from tests.test_w64_walk_model_cpu import BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flash-attention_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (the torch extension is built with one)"
    exe = str(tmp_path_factory.mktemp("w64_decode") / "w64_decode_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__=1", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "w64_decode_check.cpp"), "-o", exe])
    return exe


def test_reciprocals_equal_integer_division(checker):
    r = subprocess.run([checker, "div"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-500:] + r.stderr[-500:]
    assert int(r.stdout.split()[1]) > 5e7


def choose_units(batch, kv_heads, ratio, blocks):   # csrc/fa_launch.h
    n_groups = batch * kv_heads
    if kv_heads % 8 == 0:
        return n_groups, ratio * blocks, kv_heads // 8
    ok = lambda n: n >= 16 and ((n + 7) // 8 * 8 - n) * 8 <= n
    if ok(n_groups):
        return n_groups, ratio * blocks, 0
    if ok(n_groups * ratio):
        return n_groups * ratio, blocks, 0
    return n_groups * ratio * blocks, 1, 0


def xcd_interleave(bid, n_units, unit_size, hpx):   # csrc/fa_device.h
    xcd, slot = bid % 8, bid // 8
    j, item = slot // unit_size, slot % unit_size
    if hpx > 0:
        bb = j // hpx
        unit = bb * (8 * hpx) + xcd * hpx + (j - bb * hpx)
    else:
        unit = xcd + 8 * j
    return unit * unit_size + item if unit < n_units else -1


def model_walk(b, h, h_k, nmb, wr, grid):
    n_units, unit_size, hpx = choose_units(b, h_k, h // h_k, nmb)
    total = (n_units + 7) // 8 * 8 * unit_size
    snake = wr >= 0 and unit_size > 1 and (grid // 8) % unit_size == 0
    rows = []
    for first in range(grid):
        for rnd, vb in enumerate(range(first, total, grid)):
            bid = vb
            if snake and rnd & 1:
                item = (vb // 8) % unit_size
                bid = vb + 8 * (unit_size - 1 - 2 * item)
            w = xcd_interleave(bid, n_units, unit_size, hpx)
            if w < 0:
                rows.append((vb, rnd, -1, -1, -1))
                continue
            bh, mbr = w // nmb, w % nmb
            rows.append((vb, rnd, bh // h, bh % h, nmb - 1 - mbr if wr >= 0 else mbr))
    return (n_units, unit_size, hpx, total), rows


# (batch, heads, kv heads, sequence length, right bound, workgroups): the benchmark's shape; the two-round walk of tests/test_fwd_w64_block_code_gpu.py with and
# without grouped heads; kv heads that are no multiple of 8 (round-robin units, per-head units, one block per unit); a partially filled last round; odd everything
WALKS = [(4, 32, 32, 4096, 0, 256), (4, 32, 32, 4096, -1, 256), (2, 80, 80, 512, 0, 256), (2, 80, 20, 512, 0, 256), (2, 80, 20, 512, -1, 256),
         (3, 12, 4, 2048, 0, 256), (5, 6, 2, 1000, 0, 64), (1, 3, 1, 700, 0, 8), (7, 24, 24, 777, 17, 248), (16, 16, 16, 1024, 0, 256), (9, 40, 8, 300, -1, 128)]


@pytest.mark.parametrize("b,h,h_k,sq,wr,grid", WALKS)
def test_persistent_walk_decodes_as_the_divisions_do(checker, b, h, h_k, sq, wr, grid):
    nmb = (sq + BM - 1) // BM
    r = subprocess.run([checker, "walk"] + [str(x) for x in (b, h, h_k, nmb, wr, grid)], capture_output=True, text=True, check=True)
    lines = r.stdout.split("\n")
    head = lines[0].split()
    units, rows = model_walk(b, h, h_k, nmb, wr, grid)
    assert (int(head[1]), int(head[2]), int(head[3]), int(head[5])) == units
    got = [tuple(int(x) for x in ln.split()) for ln in lines[1:] if ln]
    assert got == rows
    real = [x[2:] for x in got if x[2] >= 0]
    assert len(real) == b * h * nmb and len(set(real)) == len(real)   # every (batch, head, query block) exactly once
