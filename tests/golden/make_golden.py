"""Generate golden vectors from the REFERENCE's own oracle (run in the build container only).

    python tests/golden/make_golden.py

Imports ``attention_ref`` from /root/reference/tests/test_util.py (the function the
reference's acceptance tests compare against, tests/test_flash_attn.py:217-304) and
torch autograd for the gradients, on CPU in fp32 (``upcast=True``), with seeded inputs.
Inputs are quantised to bf16-representable values first so that the same tensors can
be fed to the HIP kernels bit-for-bit.  Also records the fixed-``cu_seqlens`` varlen
known-answer layouts the reference tests use (tests/test_flash_attn.py:2363-2380,
tests/test_flash_attn_ck.py:1515-1560).  /root/reference is not available on the GPU
box, hence committed fixtures.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def _import_ref():
    # tests/test_util.py imports flash_attn.bert_padding -> flash_attn/__init__ -> backend module.
    # Provide an empty stand-in backend so the pure-python oracle imports on CPU.
    sys.modules.setdefault("flash_attn_2_cuda", types.ModuleType("flash_attn_2_cuda"))
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "tests"))
    import test_util  # noqa
    return test_util


CASES = [
    # name, B, Sq, Sk, H, Hk, D, causal, window, softcap, alibi
    ("mha_full_d64", 2, 96, 96, 2, 2, 64, False, (-1, -1), 0.0, False),
    ("mha_causal_d128", 1, 113, 171, 2, 2, 128, True, (-1, -1), 0.0, False),
    ("gqa_causal_sq_gt_sk", 1, 203, 113, 4, 2, 64, True, (-1, -1), 0.0, False),
    ("mqa_local_d128", 1, 128, 177, 2, 1, 128, False, (37, 11), 0.0, False),
    ("gqa_causal_window_d128", 1, 160, 160, 4, 2, 128, True, (64, 0), 0.0, False),
    # one-sided left window is written (20, Sk): the reference *test oracle* reads a literal -1 on the right as
    # "col > row + shift - 1" (tests/test_util.py:176-181) whereas the API/kernel treat it as unbounded
    # (flash_api.cpp:159-160); an explicit right bound >= Sk means the same thing to both.
    ("local_left_only_d64", 1, 99, 160, 2, 2, 64, False, (20, 160), 0.0, False),
    ("local_right_only_d64", 1, 160, 99, 2, 1, 64, False, (-1, 13), 0.0, False),
    ("tiny_sq1", 2, 1, 77, 2, 2, 128, True, (-1, -1), 0.0, False),
    ("softcap_d64", 1, 64, 96, 2, 2, 64, True, (-1, -1), 15.0, False),
    ("alibi_d64", 2, 80, 112, 2, 1, 64, True, (-1, -1), 0.0, True),
    ("d32_full", 1, 70, 70, 2, 2, 32, False, (-1, -1), 0.0, False),
    ("d96_causal", 1, 65, 129, 2, 1, 96, True, (-1, -1), 0.0, False),
    ("d256_causal", 1, 48, 80, 2, 2, 256, True, (-1, -1), 0.0, False),
]


def main():
    tu = _import_ref()
    out = {}
    for (name, B, Sq, Sk, H, Hk, D, causal, window, softcap, alibi) in CASES:
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        q = torch.randn(B, Sq, H, D, generator=g).bfloat16().float().requires_grad_()
        k = torch.randn(B, Sk, Hk, D, generator=g).bfloat16().float().requires_grad_()
        v = torch.randn(B, Sk, Hk, D, generator=g).bfloat16().float().requires_grad_()
        do = torch.randn(B, Sq, H, D, generator=g).bfloat16().float()
        bias = None
        slopes = None
        if alibi:
            slopes = (torch.rand(B, H, generator=g) * 0.3).float()
            # bias definition of tests/test_flash_attn.py:29-58 (that module needs a GPU at import,
            # :23-26, so the three lines are restated): -slope * |i + Sk - Sq - j|
            ii = torch.arange(Sq)[:, None]
            jj = torch.arange(Sk)[None, :]
            bias = -slopes[:, :, None, None] * (ii + Sk - Sq - jj).abs().float()
        o, _ = tu.attention_ref(q, k, v, None, None, bias, 0.0, None, causal=causal,
                                window_size=window, softcap=softcap)
        try:
            dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
        except RuntimeError:
            # the reference's softcap branch applies tanh in place (tests/test_util.py:234-237),
            # which autograd cannot differentiate: forward-only golden for that case.
            dq = dk = dv = None
        pre = name + "/"
        # inputs are exactly bf16-representable: store the 16-bit patterns (upper half of the fp32 word)
        for nm, t in (("q", q), ("k", k), ("v", v), ("do", do)):
            bits = t.detach().numpy().astype(np.float32).view(np.uint32)
            assert not np.any(bits & 0xFFFF)
            out[pre + nm + "_bf16bits"] = (bits >> 16).astype(np.uint16)
        out[pre + "out"] = o.detach().numpy().astype(np.float32)
        if dq is not None:
            out[pre + "dq"] = dq.numpy().astype(np.float32)
            out[pre + "dk"] = dk.numpy().astype(np.float32)
            out[pre + "dv"] = dv.numpy().astype(np.float32)
        out[pre + "meta"] = np.array([B, Sq, Sk, H, Hk, D, int(causal), window[0], window[1]], dtype=np.int64)
        out[pre + "softcap"] = np.array([softcap], dtype=np.float64)
        if slopes is not None:
            out[pre + "alibi_slopes"] = slopes.numpy()
        print(name, "out", tuple(o.shape), "max|out|", float(o.detach().abs().max()))
    _savez(os.path.join(HERE, "attention_ref_cases.npz"), out)

    # dropout: the reference oracle with an explicit keep-mask (tests/test_util.py:262-269), seeded mask
    dro = {}
    for (name, B, Sq, Sk, H, Hk, D, causal, window, pdrop) in [
            ("drop_full_d64", 1, 72, 96, 2, 2, 64, False, (-1, -1), 0.17),
            ("drop_causal_gqa_d128", 2, 65, 100, 4, 2, 128, True, (-1, -1), 0.3),
            ("drop_local_d64", 1, 96, 96, 2, 1, 64, False, (30, 10), 0.1)]:
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        q = torch.randn(B, Sq, H, D, generator=g).bfloat16().float().requires_grad_()
        k = torch.randn(B, Sk, Hk, D, generator=g).bfloat16().float().requires_grad_()
        v = torch.randn(B, Sk, Hk, D, generator=g).bfloat16().float().requires_grad_()
        do = torch.randn(B, Sq, H, D, generator=g).bfloat16().float()
        keep = torch.rand(B, H, Sq, Sk, generator=g) >= pdrop
        o, _ = tu.attention_ref(q, k, v, None, None, None, pdrop, keep, causal=causal, window_size=window)
        dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
        pre = name + "/"
        for nm, t in (("q", q), ("k", k), ("v", v), ("do", do)):
            bits = t.detach().numpy().astype(np.float32).view(np.uint32)
            dro[pre + nm + "_bf16bits"] = (bits >> 16).astype(np.uint16)
        dro[pre + "keep"] = np.packbits(keep.numpy())
        for nm, t in (("out", o), ("dq", dq), ("dk", dk), ("dv", dv)):
            dro[pre + nm] = t.detach().numpy().astype(np.float32)
        dro[pre + "meta"] = np.array([B, Sq, Sk, H, Hk, D, int(causal), window[0], window[1]], dtype=np.int64)
        dro[pre + "p"] = np.array([pdrop], dtype=np.float64)
        print(name, "out", tuple(o.shape))
    _savez(os.path.join(HERE, "dropout_ref_cases.npz"), dro)

    # documented causal mask pictures, flash_attn_interface.py:1176-1185 (1 = keep)
    pics = {
        "mask_2x5": np.array([[1, 1, 1, 1, 0], [1, 1, 1, 1, 1]], dtype=np.int8),
        "mask_5x2": np.array([[0, 0], [0, 0], [0, 0], [1, 0], [1, 1]], dtype=np.int8),
    }
    # cross-check the pictures against the reference's construct_local_mask (True = masked)
    for nm, pic in pics.items():
        sq, sk = pic.shape
        m = tu.construct_local_mask(sq, sk, (-1, 0))
        assert np.array_equal(~m.numpy(), pic.astype(bool)), nm
    # fixed cu_seqlens layouts used by reference regression tests
    pics["cu_bwd_varlen_overflow_q"] = np.array([0, 76, 110, 256], dtype=np.int32)   # test_flash_attn.py:2363
    pics["cu_bwd_varlen_overflow_k"] = np.array([0, 1, 2, 3], dtype=np.int32)
    pics["cu_seqq_zero_q"] = np.array([0, 0, 256, 512], dtype=np.int32)              # test_flash_attn_ck.py:1522-1560
    pics["cu_seqq_zero_k"] = np.array([0, 503, 768, 1536], dtype=np.int32)
    _savez(os.path.join(HERE, "known_answers.npz"), pics)
    concat_unpad_case()
    print("wrote fixtures to", HERE)


def concat_unpad_case():
    """The reference's unpad_input_for_concatenated_sequences (flash_attn/bert_padding.py) on one seeded case, inputs and outputs
    (tests/test_bert_padding_cpu.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_bert_padding", os.path.join(REF, "flash_attn", "bert_padding.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.manual_seed(1)
    mil = torch.tensor([[4, 1, 2, 0, 0, 0, 0, 0, 0], [9, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0, 0]])
    x = torch.randn(4, 9, 2, 8)
    xp, idx, cu, mx = ref.unpad_input_for_concatenated_sequences(x, mil)
    _savez(os.path.join(HERE, "concat_unpad_ref_case.npz"), dict(x=x.numpy(), attention_mask_in_length=mil.numpy(),
                                                                  hidden=xp.numpy(), indices=idx.numpy(), cu_seqlens=cu.numpy(), max_seqlen=np.array(int(mx))))


# ---------------------------------------------------------------------------------------------------------------------
# The wider matrix (tests/test_golden_matrix_{cpu,gpu}.py).  Same recipe as CASES above -- seeded CPU randn inputs stored as
# bf16 bit patterns, attention_ref(upcast=True) + autograd in fp32 -- plus, per case:
#   * inputs with |x| < 2^-14 flushed to zero, so that every value is exact in fp16 as well (one fixture, both dtypes);
#   * lse: fp32 logsumexp of the same masked scores (+inf where a row sees no key);
#   * err_pt_bf16 / err_pt_fp16: max|x_pt - x_ref| for out, dq, dk, dv, where x_pt is attention_ref(upcast=False,
#     reorder_ops=True) + autograd ON THE CPU in that dtype -- the reference's own yardstick (tests/test_flash_attn.py:1130-1132);
#   * packed batches: the two padding masks of generate_random_padding_mask, tensors stored padded (references are zero at
#     padded rows / keys);
#   * Sq >= 1024: out / dq / lse for the rows in `rows` only (first and last 128 plus every 16th), dk / dv in full.
# Sizes are a condition (README key of every file): B = 4 and six or eight query heads on every pair would be ~150 MB.  What the budget is spent on, in this order:
#   * the group split of the dK/dV kernels (fa_api.cpp bwd_gsplit_plan) on more than one query row WITH Hk = 2 and / or B = 2 -- only there the real-kv-head index
#     of a virtual head, the workspace's h_k * gs strides and the group sum's batch stride are not trivially zero: 8/2 (split 4) at B = 2 on a causal and on a
#     local pair and over three key blocks, 8/1 (split 8) on a causal and on a local (B = 2) pair, 6/2 (ratio 3: never split) and 6/1 (split 2);
#   * every pair of the reference's list, every head dim, the packed batches;
#   * the rest (one mode only for the long pairs, D = 32 wherever the head dim is not the point, B = 1) is what had to give.
# Written in shards below 1 MiB, the limit for a committed file here (one file per family would be 3 - 9 MB): <family>_NN.npz; tests/_util.load_matrix() reads a
# family back.
MATRIX = {
    # name: B, Sq, Sk, H, Hk, D, mode[, feature]          mode: full / causal / local (window drawn from the case's seed)
    "fixed": [
        ("gqa4_causal_113x203_d32", 2, 113, 203, 8, 2, 32, "causal"),
        ("gqa4_local_113x203_d59", 1, 113, 203, 4, 1, 59, "local"),
        ("gqa3_full_128x217_d40", 1, 128, 217, 6, 2, 40, "full"),
        ("mqa6_causal_128x217_d32", 1, 128, 217, 6, 1, 32, "causal"),
        ("gqa4_local_128x217_d32", 2, 128, 217, 8, 2, 32, "local"),
        ("mqa8_local_113x211_d32", 2, 113, 211, 8, 1, 32, "local"),
        ("mha_causal_113x211_d160", 1, 113, 211, 1, 1, 160, "causal"),
        ("mha_local_113x203_d192", 1, 113, 203, 1, 1, 192, "local"),
        ("mha_full_113x203_d224", 1, 113, 203, 1, 1, 224, "full"),
        ("gqa4_causal_108x256_d64", 1, 108, 256, 4, 1, 64, "causal"),
        ("mha_full_108x256_d32", 1, 108, 256, 1, 1, 32, "full"),
        ("mqa6_causal_1x147_d111", 1, 1, 147, 6, 1, 111, "causal"),
        ("gqa4_full_1x147_d64", 1, 1, 147, 8, 2, 64, "full"),
        ("gqa2_full_1x147_d160", 1, 1, 147, 2, 1, 160, "full"),
        ("gqa2_local_1x147_d192", 1, 1, 147, 2, 1, 192, "local"),
        ("mha_causal_1x147_d224", 1, 1, 147, 1, 1, 224, "causal"),
        ("mqa8_causal_256x512_d32", 1, 256, 512, 8, 1, 32, "causal"),
        ("gqa2_causal_512x256_d32", 1, 512, 256, 2, 1, 32, "causal"),
        ("mha_causal_128x128_d40", 1, 128, 128, 1, 1, 40, "causal"),      # Sq = Sk and H = Hk: the qkv-packed entry (not a pair of the reference's list either)
        ("gqa4_causal_128x640_d32", 1, 128, 640, 8, 2, 32, "causal"),      # three key blocks (not a pair of the reference's list)
        ("softcap_gqa4_causal_113x203_d32", 1, 113, 203, 4, 1, 32, "causal", ("softcap", 15.0)),
        ("softcap_gqa4_full_128x217_d32", 1, 128, 217, 4, 1, 32, "full", ("softcap", 5.0)),
        ("alibi_gqa4_causal_113x203_d32", 1, 113, 203, 4, 1, 32, "causal", ("alibi",)),
        ("alibi_gqa4_full_128x217_d64", 1, 128, 217, 4, 1, 64, "full", ("alibi",)),
    ],
    "varlen": [
        # ..., ("pad", query mask mode, key mask mode, zero_lengths)
        ("pk_mha_causal_113x203_d64", 2, 113, 203, 1, 1, 64, "causal", ("pad", "random", "random", False)),
        ("pk_mqa2_local_113x203_d64", 2, 113, 203, 2, 1, 64, "local", ("pad", "random", "third", False)),
        ("pk_mqa2_causal_108x256_d59", 2, 108, 256, 2, 1, 59, "causal", ("pad", "third", "third", False)),
        ("pk_gqa3_local_113x211_d59", 2, 113, 211, 3, 1, 59, "local", ("pad", "third", "random", False)),
        ("pk_mha_local_113x211_d59", 2, 113, 211, 1, 1, 59, "local", ("pad", "third", "third", False)),
        ("pk_mqa2_causal_zero_113x203_d64", 3, 113, 203, 2, 1, 64, "causal", ("pad", "random", "random", True)),
        ("pk_gqa2_causal_1x147_d128", 2, 1, 147, 2, 1, 128, "causal", ("pad", "random", "third", False)),
        ("pk_mha_causal_113x203_d128", 2, 113, 203, 1, 1, 128, "causal", ("pad", "third", "random", False)),
    ],
    "long": [
        ("gqa2_causal_1024x1024_d32", 1, 1024, 1024, 2, 1, 32, "causal"),
        ("mha_full_1023x1024_d32", 1, 1023, 1024, 1, 1, 32, "full"),
        ("gqa2_local_1024x1023_d32", 1, 1024, 1023, 2, 1, 32, "local"),
        ("gqa2_causal_2048x2048_d32", 1, 2048, 2048, 2, 1, 32, "causal"),
    ],
}
SHARD_BYTES = 1_000_000         # raw bytes of the arrays of one shard (compression only shrinks them): every file stays below 1 MiB
MATRIX_README = (
    "Reference-generated fixtures (tests/golden/make_golden.py, MATRIX).  Per case: q/k/v/do_bf16bits (bf16 bit patterns, every value also exact in fp16); "
    "out, dq, dk, dv, lse fp32 from the reference's attention_ref(upcast=True) + torch.autograd on the CPU (lse: logsumexp of the same masked scores, +inf for rows "
    "without a key); err_pt_bf16 / err_pt_fp16 = max|x_pt - x_ref| for (out, dq, dk, dv) with x_pt from attention_ref(upcast=False, reorder_ops=True) + autograd in "
    "that dtype on the CPU (both dtypes ran for every case: no op was missing); meta = B, Sq, Sk, H, Hk, D, causal, window_left, window_right; rows (only where "
    "Sq >= 1024) = the query rows out / dq / lse are stored for; qmask / kmask (packed cases) = padding masks, tensors stored padded.  Softcap cases: the reference's "
    "in-place tanh is not differentiable, so dq / dk / dv are the project's fp64 oracle's (bwd_from_oracle = 1) and the gradient entries of err_pt_* are NaN.  "
    "Arrays above the shard size are stored raveled as <key>__partN with <key>__shape.")


def _flush(t):
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def _sample_rows(Sq):
    return np.array(sorted(set(range(128)) | set(range(Sq - 128, Sq)) | set(range(0, Sq, 16))), dtype=np.int64)


def _matrix_case(tu, orc, name, B, Sq, Sk, H, Hk, D, mode, feat=()):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    q, k, v, do = (_flush(torch.randn(*s, generator=g).bfloat16().float()) for s in ((B, Sq, H, D), (B, Sk, Hk, D), (B, Sk, Hk, D), (B, Sq, H, D)))
    causal, window = mode == "causal", (-1, -1)
    if mode == "local":   # explicit bounds on both sides (see local_left_only_d64 above)
        window = tuple(int(x) for x in torch.randint(0, Sk, (2,), generator=g))
    softcap, slopes, bias, qmask, kmask = 0.0, None, None, None, None
    if feat and feat[0] == "softcap":
        softcap = feat[1]
    if feat and feat[0] == "alibi":
        slopes = (torch.rand(B, H, generator=g) * 0.3).float()
        bias = -slopes[:, :, None, None] * (torch.arange(Sq)[:, None] + Sk - Sq - torch.arange(Sk)[None, :]).abs().float()
    if feat and feat[0] == "pad":
        torch.manual_seed(sum(map(ord, name)))   # generate_random_padding_mask draws from the global generator
        qmask = tu.generate_random_padding_mask(Sq, B, "cpu", mode=feat[1], zero_lengths=feat[3])
        kmask = tu.generate_random_padding_mask(Sk, B, "cpu", mode=feat[2], zero_lengths=feat[3])

    def run(dtype, upcast):
        qq, kk, vv = (t.clone().to(dtype).requires_grad_() for t in (q, k, v))
        o, _ = tu.attention_ref(qq, kk, vv, qmask, kmask, bias if bias is None else bias.to(dtype), 0.0, None, causal=causal, window_size=window,
                                softcap=softcap, upcast=upcast, reorder_ops=not upcast)
        if softcap > 0.0:
            return [o.detach().float()] + [None] * 3
        return [o.detach().float()] + [x.float() for x in torch.autograd.grad(o, (qq, kk, vv), do.to(dtype))]

    ref = run(torch.float32, True)
    case = {}
    if softcap > 0.0:
        ref[1:] = [torch.from_numpy(x).float() for x in orc.attention_bwd(do, q, k, v, None, None, None, causal, window, softcap)[:3]]
        case["bwd_from_oracle"] = np.array([1], dtype=np.int64)
    for dtype, key in ((torch.bfloat16, "err_pt_bf16"), (torch.float16, "err_pt_fp16")):
        pt = run(dtype, False)
        case[key] = np.array([float("nan") if x is None else float((x - r).abs().max()) if r.numel() else 0.0 for x, r in zip(pt, ref)], dtype=np.float64)
    # LSE: the three lines, on the scores attention_ref masks (tests/test_util.py:232-253)
    w = (window[0], 0) if causal else window
    s = torch.einsum("bthd,bshd->bhts", q / D ** 0.5, k.repeat_interleave(H // Hk, dim=2))
    if softcap > 0.0:
        s = softcap * torch.tanh(s / softcap)
    if kmask is not None:
        s = s.masked_fill(~kmask[:, None, None, :], float("-inf"))
    if w[0] >= 0 or w[1] >= 0:
        s = s.masked_fill(tu.construct_local_mask(Sq, Sk, w, qmask, kmask, "cpu"), float("-inf"))
    if bias is not None:
        s = s + bias
    lse = torch.logsumexp(s, dim=-1)
    lse = torch.where(torch.isneginf(lse), torch.full_like(lse, float("inf")), lse)
    for nm, t in (("q", q), ("k", k), ("v", v), ("do", do)):
        bits = t.numpy().view(np.uint32)
        assert not np.any(bits & 0xFFFF)
        case[nm + "_bf16bits"] = (bits >> 16).astype(np.uint16)
    out, dq, dk, dv = (t.numpy().astype(np.float32) for t in ref)
    lse = lse.numpy().astype(np.float32)
    if Sq >= 1024:
        rows = _sample_rows(Sq)
        out, dq, lse, case["rows"] = out[:, rows], dq[:, rows], lse[:, :, rows], rows
    case.update(out=out, dq=dq, dk=dk, dv=dv, lse=lse)
    case["meta"] = np.array([B, Sq, Sk, H, Hk, D, int(causal), window[0], window[1]], dtype=np.int64)
    case["softcap"] = np.array([softcap], dtype=np.float64)
    if slopes is not None:
        case["alibi_slopes"] = slopes.numpy()
    if qmask is not None:
        case["qmask"], case["kmask"] = qmask.numpy(), kmask.numpy()
    assert all(np.isfinite(case[x]).all() for x in ("out", "dq", "dk", "dv")), name
    return case


def _same_arrays(path, arrays):
    if not os.path.exists(path):
        return False
    with np.load(path) as z:
        return sorted(z.files) == sorted(arrays) and all(
            z[k].dtype == np.asarray(a).dtype and z[k].shape == np.asarray(a).shape and z[k].tobytes() == np.asarray(a).tobytes() for k, a in arrays.items())


def _savez(path, arrays):
    """np.savez_compressed, but a file whose arrays are already these is left alone (the zip container carries time stamps)."""
    if _same_arrays(path, arrays):
        return
    np.savez_compressed(path, **arrays)


def _save_sharded(family, arrays):
    shards, cur, used = [], {}, 0
    for key, a in arrays.items():
        a = np.ascontiguousarray(a)
        parts = {key: a}
        if a.nbytes > SHARD_BYTES:
            n = -(-a.nbytes // SHARD_BYTES)
            parts = {"%s__part%d" % (key, i): p for i, p in enumerate(np.array_split(a.ravel(), n))}
            parts[key + "__shape"] = np.array(a.shape, dtype=np.int64)
        for kk, p in parts.items():
            if cur and used + p.nbytes > SHARD_BYTES:
                shards.append(cur)
                cur, used = {}, 0
            cur[kk] = p
            used += p.nbytes
    shards.append(cur)
    import glob
    want = [os.path.join(HERE, "ref_matrix_%s_%02d.npz" % (family, i)) for i in range(len(shards))]
    for stale in set(glob.glob(os.path.join(HERE, "ref_matrix_%s_*.npz" % family))) - set(want):
        os.remove(stale)
    for path, sh in zip(want, shards):
        _savez(path, sh)
    return want


def matrix():
    tu = _import_ref()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import attention_oracle as orc
    total = 0
    for family, cases in MATRIX.items():
        arrays = {"README": np.array(MATRIX_README)}
        for row in cases:
            case = _matrix_case(tu, orc, *row[:8], feat=row[8] if len(row) > 8 else ())
            arrays.update({row[0] + "/" + k: a for k, a in case.items()})
            print(row[0], "err_pt_bf16", case["err_pt_bf16"], "err_pt_fp16", case["err_pt_fp16"])
        sizes = [os.path.getsize(p) for p in _save_sharded(family, arrays)]
        assert max(sizes) < (1 << 20), sizes
        total += sum(sizes)
        print(family, len(cases), "cases,", len(sizes), "files,", sum(sizes), "bytes")
    print("matrix total", total, "bytes")
    assert total <= 18_000_000


if __name__ == "__main__":
    main()
    matrix()
