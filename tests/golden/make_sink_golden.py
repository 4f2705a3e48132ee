"""Generate the attention-sink fixture from the REFERENCE's own oracle (run where the reference checkout is available, on the CPU).

    python tests/golden/make_sink_golden.py      ->  tests/golden/sink_ref_cases_NN.npz   (tests/_sink_ref.py load_cases() reads them back)

Imports ``attention_ref`` from the reference's flash_attn/utils/testing.py (the oracle its tests/cute/test_flash_attn.py compares the learnable sink against),
loaded the way make_golden.py loads the reference's test utilities: a stub for ``flash_attn_2_cuda``, nothing of the reference's text stored.  Per case:
  * q / k / v / do_bf16bits: seeded randn, rounded to bf16 with |x| < 2^-14 flushed to zero, so that every value is exact in fp16 as well (one fixture, both
    dtypes); sink: fp32 values that are exact in bf16 and fp16 (N(0, 2^2), or the pinned set -inf, -30, 0, +30);
  * out, dq, dk, dv, dsink: fp32, attention_ref(learnable_sink=sink, upcast=True) + torch.autograd;
  * lse: the logsumexp of the same masked (and soft-capped) scores with the sink joined -- the sink itself on a row without a visible key;
  * err_pt_bf16 / err_pt_fp16: max|x_pt - x_ref| for (out, dq, dk, dv, dsink), x_pt from attention_ref(upcast=False, reorder_ops=True) + autograd in that dtype
    with the sink cast to it -- the reference's own yardstick;
  * meta = H, Hk, D, causal, window_left, window_right; softcap; packed; qlens / klens: the sequences.  A packed case stores (total, H, D) tensors and is run
    through the reference one sequence at a time (B = 1, no padding masks), the gradients of the sink summed over the sequences by autograd.
The fixture must leave the kernels room: tests/_sink_ref.py's stand-in (the kernels' roundings, in torch) has to stay within HALF of each rule's allowance on
every case, in every realisation of the rounding noise that it draws (STANDIN_VARIANTS; sixteen for dsink, DSINK_VARIANTS): per case the seed is name + 1000 * salt for the first salt on which it does (stored), and the script refuses to write a fixture without one.  Files stay below 1 MiB each.
"""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
SHARD_BYTES = 900_000
INF = math.inf
MAX_SALT = 40000

CASES = [
    # name, qlens, klens, H, Hk, D, causal, window, softcap, sinks ("randn" or a list), packed
    ("gqa4_causal_113x203_d40", [113], [203], 8, 2, 40, True, (-1, -1), 0.0, "randn", False),
    ("mqa8_causal_140x77_d64", [140], [77], 8, 1, 64, True, (-1, -1), 0.0, "randn", False),                   # Sq > Sk: 63 rows without a key
    ("mqa4_window31_257x257_d64", [257], [257], 4, 1, 64, False, (31, 0), 0.0, "randn", False),
    ("gqa8_window31_65x129_d64", [65], [129], 16, 2, 64, False, (31, 0), 0.0, "randn", False),
    ("mha_full_64x300_d128", [64], [300], 1, 1, 128, False, (-1, -1), 0.0, "randn", False),
    ("gqa2_softcap30_causal_113x113_d40", [113] * 2, [113] * 2, 4, 2, 40, True, (-1, -1), 30.0, "randn", False),
    ("mqa4_decode_1x515_d64", [1], [515], 4, 1, 64, False, (-1, -1), 0.0, "randn", False),
    ("mha_causal_113x113_d256", [113], [113], 1, 1, 256, True, (-1, -1), 0.0, "randn", False),
    ("pinned_gqa2_causal_113x257_d64", [113], [257], 4, 2, 64, True, (-1, -1), 0.0, [-INF, -30.0, 0.0, 30.0], False),
    ("pinned_mqa4_causal_140x77_d64", [140], [77], 4, 1, 64, True, (-1, -1), 0.0, [-30.0, 0.0, 30.0, 0.5], False),        # ... with rows without a key (no -inf: the reference is NaN there)
    ("pk_gqa2_causal_zero_d64", [113, 0, 57], [203, 40, 80], 4, 2, 64, True, (-1, -1), 0.0, "randn", True),    # a sequence with keys and no query
    ("pk_mqa2_window31_d128", [200, 31, 0], [77, 257, 0], 2, 1, 128, True, (31, 0), 0.0, "randn", True),       # rows without a key, an empty sequence
]


def _import_ref():
    sys.modules.setdefault("flash_attn_2_cuda", types.ModuleType("flash_attn_2_cuda"))
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("ref_testing", os.path.join(REF, "flash_attn", "utils", "testing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _flush(t):
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def _ref_window(causal, window):
    """This package's (-1 = unbounded) to the reference's (None = unbounded); causal sets the right bound to 0 in both."""
    wl, wr = (None if w < 0 else w for w in window)
    if wl is not None and wr is None and not causal:
        wr = 1 << 20       # (the reference needs an explicit right bound beside a left one)
    return wl, wr


def _case(tm, salt, name, qlens, klens, H, Hk, D, causal, window, softcap, sinks, packed):
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 1000 * salt)
    tq, tk = sum(qlens), sum(klens)
    q, k, v, do = (_flush(torch.randn(*s, generator=g).bfloat16().float()) for s in ((tq, H, D), (tk, Hk, D), (tk, Hk, D), (tq, H, D)))
    sink = (torch.randn(H, generator=g) * 2.0).bfloat16().float() if sinks == "randn" else torch.tensor(sinks, dtype=torch.float32)
    assert sink.shape == (H,) and torch.equal(sink.half().float(), sink)
    cq, ck = np.concatenate([[0], np.cumsum(qlens)]), np.concatenate([[0], np.cumsum(klens)])
    seqs = [(slice(int(cq[i]), int(cq[i + 1])), slice(int(ck[i]), int(ck[i + 1]))) for i in range(len(qlens))]
    rw = _ref_window(causal, window)

    def run(dtype, upcast):
        qq, kk, vv = (t.clone().to(dtype).requires_grad_() for t in (q, k, v))
        ss = sink.clone().to(dtype).requires_grad_()
        outs, loss = [], 0.0
        for sq_, sk_ in seqs:
            if sq_.stop == sq_.start:
                continue
            o, _ = tm.attention_ref(qq[None, sq_], kk[None, sk_], vv[None, sk_], causal=causal, window_size=rw, learnable_sink=ss, softcap=softcap,
                                    upcast=upcast, reorder_ops=not upcast)
            outs.append(o[0])
            loss = loss + (o[0].float() * do[sq_]).sum() if upcast else loss + (o[0] * do[sq_].to(dtype)).sum()
        grads = torch.autograd.grad(loss, (qq, kk, vv, ss), allow_unused=True)
        grads = [torch.zeros_like(t) if x is None else x for x, t in zip(grads, (qq, kk, vv, ss))]
        return [torch.cat(outs).detach().float()] + [x.float() for x in grads]

    ref = run(torch.float32, True)
    case = {}
    for dtype, key in ((torch.bfloat16, "err_pt_bf16"), (torch.float16, "err_pt_fp16")):
        pt = run(dtype, False)
        case[key] = np.array([float((x - r).abs().max()) for x, r in zip(pt, ref)], dtype=np.float64)
    # lse': the scores attention_ref masks, with the sink joined
    lse = torch.zeros(H, tq)
    for sq_, sk_ in seqs:
        Sq, Sk = sq_.stop - sq_.start, sk_.stop - sk_.start
        if Sq == 0:
            continue
        s = torch.einsum("thd,shd->hts", q[sq_] / math.sqrt(D), k[sk_].repeat_interleave(H // Hk, dim=1))
        if softcap > 0:
            s = torch.tanh(s / softcap) * softcap
        w = (rw[0], 0) if causal else rw
        if w[0] is not None or w[1] is not None:
            s = s.masked_fill(tm.construct_local_mask(Sq, Sk, w)[None], -INF)
        lse[:, sq_] = torch.logsumexp(torch.cat([s, sink[:, None, None].expand(H, Sq, 1)], dim=-1), dim=-1)
    B = len(qlens)
    shape = (lambda t, n: t) if packed else (lambda t, n: t.reshape(B, n // B, *t.shape[1:]))
    for nm, t, n in (("q", q, tq), ("k", k, tk), ("v", v, tk), ("do", do, tq)):
        bits = shape(t, n).contiguous().numpy().view(np.uint32)
        assert not np.any(bits & 0xFFFF)
        case[nm + "_bf16bits"] = (bits >> 16).astype(np.uint16)
    out, dq, dk, dv, dsink = ref
    case.update(out=shape(out, tq).numpy(), dq=shape(dq, tq).numpy(), dk=shape(dk, tk).numpy(), dv=shape(dv, tk).numpy(), dsink=dsink.numpy(), sink=sink.numpy(),
                lse=(lse if packed else lse.view(H, B, -1).transpose(0, 1).contiguous()).numpy())
    case["meta"] = np.array([H, Hk, D, int(causal), window[0], window[1]], dtype=np.int64)
    case["softcap"] = np.array([softcap], dtype=np.float64)
    case["packed"] = np.array([int(packed)], dtype=np.int64)
    case["qlens"], case["klens"] = np.array(qlens, dtype=np.int64), np.array(klens, dtype=np.int64)
    assert all(np.isfinite(case[x]).all() for x in ("out", "dq", "dk", "dv", "dsink")), name
    return case


def _save_sharded(arrays):
    shards, cur, used = [], {}, 0
    for key, a in arrays.items():
        a = np.ascontiguousarray(a)
        assert a.nbytes <= SHARD_BYTES, (key, a.nbytes)
        if cur and used + a.nbytes > SHARD_BYTES:
            shards.append(cur)
            cur, used = {}, 0
        cur[key] = a
        used += a.nbytes
    shards.append(cur)
    import glob
    want = [os.path.join(HERE, "sink_ref_cases_%02d.npz" % i) for i in range(len(shards))]
    for stale in set(glob.glob(os.path.join(HERE, "sink_ref_cases*.npz"))) - set(want):
        os.remove(stale)
    for path, sh in zip(want, shards):
        np.savez_compressed(path, **sh)
    return want


def _find(row):
    """The first seed (name + 1000 * salt) of one case on which the stand-in keeps to half of every allowance, in both dtypes."""
    torch.set_num_threads(1)
    tm = _import_ref()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests import _sink_ref as sr
    for salt in range(MAX_SALT):
        case = _case(tm, salt, *row)
        worst, ok = {}, True
        for variant in sr.DSINK_VARIANTS:          # (stops at the first realisation that is out: most seeds fall early)
            for dtype in (torch.bfloat16, torch.float16):
                res = sr.compare(case, sr.standin(case, dtype, variant=variant), dtype)
                for nm, x in res.items():
                    if nm == "dsink" or variant in sr.STANDIN_VARIANTS:
                        worst[nm] = max(worst.get(nm, 0.0), x)
            ok = all(worst[nm] <= 0.5 for nm in sr.QUANTITIES) and worst["lse"] < sr.LSE_TOL / 2
            if not ok:
                break
        if ok:
            print(row[0], "salt", salt, "err_pt_bf16", case["err_pt_bf16"], "err_pt_fp16", case["err_pt_fp16"], "stand-in / allowance", {k: round(x, 3) for k, x in worst.items()},
                  flush=True)
            case["salt"] = np.array([salt], dtype=np.int64)
            return case
    raise SystemExit("%s: no seed below salt %d keeps the stand-in to half of every allowance" % (row[0], MAX_SALT))


def main():
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(min(len(CASES), os.cpu_count() or 1)) as pool:          # the cases are independent: one process each
        found = pool.map(_find, CASES, chunksize=1)
    arrays = {}
    for row, case in zip(CASES, found):
        arrays.update({row[0] + "/" + k: a for k, a in case.items()})
    sizes = [os.path.getsize(p) for p in _save_sharded(arrays)]
    assert max(sizes) < (1 << 20), sizes
    print(len(CASES), "cases,", len(sizes), "files,", sum(sizes), "bytes")


if __name__ == "__main__":
    main()
