"""libfa_gfx950_quant.so on the GPU, bit for bit against the CPU reference (tests/_quant_ref.py): inputs are built on the CPU with a seeded generator, the e4m3
bytes are compared as uint8 and the descales with torch.equal -- both paths (two-pass, one-launch), packed batches, static / dynamic / mixed calls, strided
layouts, the quantising append against reference quantisation + the existing e4m3 fa_kvcache_append, the consumers end to end, and a HIP-graph capture."""
import ctypes as C

import pytest
import torch

from tests._quant_ref import FP8, quant_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, HK = 2, 2


def _rand(shape, dtype, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _same_bytes(y_gpu, y_ref):
    return torch.equal(y_gpu.cpu().view(torch.uint8), y_ref.view(torch.uint8))


def _check(got, ref):
    for (y, ds), (yr, dsr) in zip(got, ref):
        assert y.dtype == FP8 and y.is_contiguous() and ds.dtype == torch.float32
        assert torch.equal(ds.cpu(), dsr), (ds.cpu(), dsr)
        assert _same_bytes(y, yr), int((y.cpu().view(torch.uint8) != yr.view(torch.uint8)).sum())


def _raw_quant(xs, ys, dss, static, hk, path=0, cus=None):
    """fa_quant_e4m3 on caller-made outputs (the Python function allocates its own): xs / ys / dss are lists of GPU tensors or views."""
    from flash_attn_amd import _cabi_quant as q
    lib = q.load()
    a = q.FaQuantParams()
    x0 = xs[0]
    cus = cus or [None] * len(xs)
    batch = x0.shape[0] if cus[0] is None else cus[0].numel() - 1
    a.n_tensors, a.b, a.h_k, a.d, a.dtype, a.path = len(xs), batch, hk, x0.shape[-1], int(x0.dtype == torch.bfloat16), path
    for i, (x, y, ds, st, cu) in enumerate(zip(xs, ys, dss, static, cus)):
        t = a.t[i]
        t.x, t.y, t.descale, t.cu_seqlens = x.data_ptr(), y.data_ptr(), ds.data_ptr(), (cu.data_ptr() if cu is not None else None)
        o = 0 if cu is not None else 1
        if cu is None:
            t.x_batch_stride, t.y_batch_stride = x.stride(0), y.stride(0)
        t.x_row_stride, t.x_head_stride, t.y_row_stride, t.y_head_stride = x.stride(o), x.stride(o + 1), y.stride(o), y.stride(o + 1)
        t.descale_batch_stride, t.descale_head_stride = ds.stride(0), ds.stride(1)
        t.heads, t.rows, t.is_static = x.shape[-2], x.shape[o], int(st)
    nbytes = lib.fa_quant_workspace_bytes(C.byref(a))
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=DEV)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    q.check(lib.fa_quant_e4m3(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [48, 64, 128])
@pytest.mark.parametrize("S", [1, 37, 1000])
def test_fixed_length_both_paths(S, D, dtype):
    """q (4 heads), k and v (2 heads) in one call, H / Hk = 4 / 2.  S = 1000 makes a group span several workgroups; S = 1 and 37 fit the one-launch kernel."""
    from flash_attn_amd import quantize_fp8
    q, k, v = _rand((B, S, 4, D), dtype, 1), _rand((B, S, HK, D), dtype, 2, 0.5), _rand((B, S, HK, D), dtype, 3, 30.0)
    ref = [quant_ref(t, HK) for t in (q, k, v)]
    legal = [1] + ([2] if S * 2 * D <= 16384 else [])
    for path in [0] + legal:
        _check(quantize_fp8(q.to(DEV), k.to(DEV), v.to(DEV), num_heads_k=HK, path=path), ref)
    if 2 not in legal:
        with pytest.raises(RuntimeError, match="exceeds the one-launch bound"):
            quantize_fp8(q.to(DEV), num_heads_k=HK, path=2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_decode_query(dtype):
    """The decode step's q: one row, 8 query heads on one KV head."""
    from flash_attn_amd import quantize_fp8
    q = _rand((3, 1, 8, 128), dtype, 4)
    ref = [quant_ref(q, 1)]
    for path in (0, 1, 2):
        _check(quantize_fp8(q.to(DEV), num_heads_k=1, path=path), ref)


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("S,path", [(5, 2), (5, 1), (300, 1)])
def test_planted_maximum_at_the_groups_edges(S, path, where):
    """The largest magnitude sits in the group's first element, or in the last element of the last row of its last head, with either sign: a reduction that
    drops an edge gets the descale wrong.  (300 rows: the group spans three workgroup tiles.)"""
    from flash_attn_amd import quantize_fp8
    H, D = 4, 64
    x = _rand((B, S, H, D), torch.bfloat16, 6, 0.25).clamp(-1, 1)
    for b in range(B):
        for g in range(HK):
            val = 7.5 if (b + g) % 2 else -7.5
            if where == "first":
                x[b, 0, g * 2, 0] = val
            else:
                x[b, S - 1, g * 2 + 1, D - 1] = val
    ref = quant_ref(x, HK)
    assert torch.equal(ref[1], torch.full((B, HK), 7.5 / 448))
    _check(quantize_fp8(x.to(DEV), num_heads_k=HK, path=path), [ref])


def test_packed_batch_with_an_empty_entry():
    from flash_attn_amd import quantize_fp8
    lens = [0, 5, 70, 1]
    cu = [0, 0, 5, 75, 76]
    q, k, v = _rand((76, 4, 64), torch.bfloat16, 7), _rand((76, 2, 64), torch.bfloat16, 8), _rand((76, 2, 64), torch.float32, 9).to(torch.bfloat16)
    ref = [quant_ref(t, HK, cu_seqlens=cu) for t in (q, k, v)]
    assert ref[0][1][0].tolist() == [1.0, 1.0]
    cu_d = torch.tensor(cu, dtype=torch.int32, device=DEV)
    got = quantize_fp8(q.to(DEV), k.to(DEV), v.to(DEV), num_heads_k=HK, cu_seqlens_q=cu_d, cu_seqlens_k=cu_d)
    _check(got, ref)
    assert got[0][1][0].tolist() == [1.0, 1.0] and len(lens) == got[0][1].shape[0]
    with pytest.raises(RuntimeError, match="packed tensor always takes the two-pass path"):
        quantize_fp8(q.to(DEV), num_heads_k=HK, cu_seqlens_q=cu_d, path=2)


@pytest.mark.parametrize("S,path", [(37, 2), (37, 1), (600, 1)])
def test_static_mode_saturates_and_leaves_the_descale_alone(S, path):
    from flash_attn_amd import quantize_fp8
    g = torch.Generator().manual_seed(10)
    ds = torch.rand(B, HK, generator=g) * 1.95 + 0.05
    x = _rand((B, S, 4, 64), torch.bfloat16, 11, 300.0)               # far beyond 448 * descale
    ref = quant_ref(x, HK, descale=ds)
    ds_d = ds.to(DEV)
    (y, ds_out), = quantize_fp8(x.to(DEV), num_heads_k=HK, q_descale=ds_d, path=path)
    assert ds_out is ds_d and torch.equal(ds_d.cpu(), ds)
    assert _same_bytes(y, ref[0])
    by = y.cpu().view(torch.uint8)
    assert (by == 0x7E).any() and (by == 0xFE).any() and not ((by & 0x7F) == 0x7F).any()


def test_mixed_call_dynamic_q_static_kv():
    from flash_attn_amd import quantize_fp8
    g = torch.Generator().manual_seed(12)
    kd, vd = torch.rand(B, HK, generator=g) + 0.05, torch.rand(B, HK, generator=g) + 0.05
    q, k, v = _rand((B, 1, 8, 128), torch.float16, 13), _rand((B, 1, HK, 128), torch.float16, 14, 100.0), _rand((B, 1, HK, 128), torch.float16, 15, 100.0)
    ref = [quant_ref(q, HK), quant_ref(k, HK, descale=kd), quant_ref(v, HK, descale=vd)]
    for path in (0, 1, 2):
        _check(quantize_fp8(q.to(DEV), k.to(DEV), v.to(DEV), num_heads_k=HK, k_descale=kd.to(DEV), v_descale=vd.to(DEV), path=path), ref)


@pytest.mark.parametrize("path", [1, 2])
def test_strided_inputs(path):
    """A (B, H, S, D) buffer seen as (B, S, H, D), the q / k / v slices of one fused projection (row stride 3 H D), heads padded to D + 8, and a descale
    tensor that is the transpose of an (Hk, B) buffer; the inputs are not written."""
    from flash_attn_amd import quantize_fp8
    S, H, D = 19, 4, 64
    qkv = _rand((B, S, 3, H, D), torch.bfloat16, 16)
    qkv_d = qkv.to(DEV)
    ref = [quant_ref(qkv[:, :, i], HK) for i in range(3)]
    _check(quantize_fp8(qkv_d[:, :, 0], qkv_d[:, :, 1], qkv_d[:, :, 2], num_heads_k=HK, path=path), ref)
    assert torch.equal(qkv_d.cpu(), qkv)
    bhsd = _rand((B, H, S, D), torch.bfloat16, 17)
    padded = _rand((B, S, H, D + 8), torch.bfloat16, 18)
    dsT = (torch.rand(HK, B, generator=torch.Generator().manual_seed(19)) + 0.1)
    ref = [quant_ref(bhsd.transpose(1, 2), HK), quant_ref(padded[..., :D], HK, descale=dsT.t())]
    dsT_d = dsT.to(DEV)
    got = quantize_fp8(bhsd.to(DEV).transpose(1, 2), padded.to(DEV)[..., :D], num_heads_k=HK, k_descale=dsT_d.t(), path=path)
    _check(got, ref)
    assert torch.equal(dsT_d.cpu(), dsT)


@pytest.mark.parametrize("path", [1, 2])
def test_outputs_inside_a_poisoned_arena(path):
    """y is a view with padded heads in the middle of a poisoned buffer, the dynamic descale the transpose of an (Hk, B) buffer inside another: every byte
    outside the two tensors keeps its poison."""
    S, H, D = 19, 4, 64
    x = _rand((B, S, H, D), torch.bfloat16, 20)
    yr, dsr = quant_ref(x, HK)
    arena = torch.full((B * S * H * (D + 16) + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    y = arena[32:32 + B * S * H * (D + 16)].view(B, S, H, D + 16)[..., :D]
    ds_arena = torch.full((HK * B + 4,), -7.0, dtype=torch.float32, device=DEV)
    ds = ds_arena[2:2 + HK * B].view(HK, B).t()
    _raw_quant([x.to(DEV)], [y], [ds], [False], HK, path=path)
    assert torch.equal(y.cpu(), yr.view(torch.uint8)) and torch.equal(ds.cpu(), dsr)
    mask = torch.ones_like(arena, dtype=torch.bool)
    mask[32:32 + B * S * H * (D + 16)].view(B, S, H, D + 16)[..., :D] = False
    assert bool((arena[mask] == 0xA5).all())
    assert ds_arena[:2].tolist() == [-7.0, -7.0] and ds_arena[-2:].tolist() == [-7.0, -7.0]


def _byte_append(kc, vc, k8, v8, lens, cache_batch_idx=None, block_table=None):
    """The existing e4m3 append of libfa_gfx950.so (a byte copy)."""
    from flash_attn_amd import _cabi
    lib = _cabi.load()
    ap = _cabi.FaKvAppendParams()
    ap.knew, ap.vnew, ap.kcache, ap.vcache = k8.data_ptr(), v8.data_ptr(), kc.data_ptr(), vc.data_ptr()
    for nm, t in (("knew", k8), ("vnew", v8), ("kcache", kc), ("vcache", vc)):
        setattr(ap, nm + "_batch_stride", t.stride(0)); setattr(ap, nm + "_row_stride", t.stride(1)); setattr(ap, nm + "_head_stride", t.stride(2))
    ap.seqlens_k = lens.data_ptr()
    ap.cache_batch_idx = cache_batch_idx.data_ptr() if cache_batch_idx is not None else None
    if block_table is not None:
        ap.block_table, ap.block_table_batch_stride, ap.page_block_size = block_table.data_ptr(), block_table.stride(0), kc.shape[1]
    ap.b, ap.seqlen_new, ap.h_k, ap.d, ap.dtype = k8.shape[0], k8.shape[1], k8.shape[2], k8.shape[3], _cabi.FA_DTYPE_FP8_E4M3
    _cabi.check(lib.fa_kvcache_append(C.byref(ap), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("s_new", [1, 3])
@pytest.mark.parametrize("mode", ["contiguous", "cache_batch_idx", "paged"])
def test_quantising_append_equals_reference_quantisation_plus_byte_append(mode, s_new, dtype):
    """Entries at lengths [0, 3, 255, 256]: with three new rows one of them crosses the page edge.  The cache starts as poison; afterwards it equals, byte for
    byte, the poison cache the existing e4m3 append wrote the reference-quantised rows into -- so the rows that were not appended are unchanged too."""
    from flash_attn_amd import kvcache_append_fp8
    Bn, D = 4, 64
    g = torch.Generator().manual_seed(21)
    lens = torch.tensor([0, 3, 255, 256], dtype=torch.int32, device=DEV)
    k, v = _rand((Bn, s_new, HK, D), dtype, 22, 40.0), _rand((Bn, s_new, HK, D), dtype, 23, 40.0)
    kd, vd = torch.rand(Bn, HK, generator=g) * 1.95 + 0.05, torch.rand(Bn, HK, generator=g) * 1.95 + 0.05
    k8, v8 = quant_ref(k, HK, descale=kd)[0].to(DEV), quant_ref(v, HK, descale=vd)[0].to(DEV)
    idx = bt = None
    if mode == "paged":
        shape = (8, 256, HK, D)
        bt = torch.randperm(8, generator=g).to(torch.int32).reshape(Bn, 2).to(DEV)
    else:
        shape = (Bn, 512, HK, D)
        if mode == "cache_batch_idx":
            idx = torch.tensor([2, 0, 3, 1], dtype=torch.int32, device=DEV)
    poison = (torch.arange(shape[0] * shape[1] * HK * D, dtype=torch.int64) * 37 % 251).to(torch.uint8).reshape(shape)
    kc_ref, vc_ref = poison.to(DEV).view(FP8), poison.flip(0).contiguous().to(DEV).view(FP8)
    kc, vc = kc_ref.clone(), vc_ref.clone()
    _byte_append(kc_ref, vc_ref, k8, v8, lens, idx, bt)
    kvcache_append_fp8(kc, vc, k.to(DEV), v.to(DEV), lens, kd.to(DEV), vd.to(DEV), cache_batch_idx=idx, block_table=bt)
    torch.cuda.synchronize()
    assert torch.equal(kc.view(torch.uint8), kc_ref.view(torch.uint8)) and torch.equal(vc.view(torch.uint8), vc_ref.view(torch.uint8))
    assert not torch.equal(kc.view(torch.uint8).cpu(), poison)


def test_consumers_see_the_same_bits_end_to_end():
    """Quantise here, run fa_fwd_kvcache_fp8 (one query row against 300 keys, unsplit and split) and fa_fwd_fp8 (165 x 165, causal): out and lse equal the
    same calls on the reference-quantised inputs exactly -- the quantisation is bit-exact, so there is nothing to tolerate."""
    from flash_attn_amd import backend as be, quantize_fp8
    H, D = 8, 128
    for Sq, Sk in ((1, 300), (165, 165)):
        q, k, v = _rand((B, Sq, H, D), torch.bfloat16, 24), _rand((B, Sk, HK, D), torch.bfloat16, 25), _rand((B, Sk, HK, D), torch.bfloat16, 26)
        ref = [quant_ref(t, HK) for t in (q, k, v)]
        got = quantize_fp8(q.to(DEV), k.to(DEV), v.to(DEV), num_heads_k=HK)
        (q8, qd), (k8, kd), (v8, vd) = got
        (q8r, qdr), (k8r, kdr), (v8r, vdr) = [(y.to(DEV), ds.to(DEV)) for y, ds in ref]
        if Sq == 1:
            lens = torch.tensor([300, 211], dtype=torch.int32, device=DEV)
            for splits in (1, 3):
                a = be.fwd_kvcache_fp8(q8, k8, v8, None, None, lens, None, None, None, qd, kd, vd, D ** -0.5, False, -1, -1, splits)
                b = be.fwd_kvcache_fp8(q8r, k8r, v8r, None, None, lens, None, None, None, qdr, kdr, vdr, D ** -0.5, False, -1, -1, splits)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        else:
            a = be.fwd_fp8(q8, k8, v8, None, qd, kd, vd, D ** -0.5, True, -1, -1)
            b = be.fwd_fp8(q8r, k8r, v8r, None, qdr, kdr, vdr, D ** -0.5, True, -1, -1)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            assert bool(torch.isfinite(a[0].float()).all())


def test_two_runs_give_identical_bytes():
    from flash_attn_amd import quantize_fp8
    x = _rand((B, 1000, 4, 128), torch.bfloat16, 27).to(DEV)
    (y1, d1), = quantize_fp8(x, num_heads_k=HK)
    (y2, d2), = quantize_fp8(x, num_heads_k=HK)
    assert torch.equal(y1.view(torch.uint8), y2.view(torch.uint8)) and torch.equal(d1, d2)


def test_graph_capture_of_a_decode_step():
    """One torch.cuda.graph holds quantize_fp8 (dynamic q, static k / v through the two-pass path, so the scratch clear is captured too) followed by
    kvcache_append_fp8 -- a linear chain.  It is replayed twice on new contents of the same input buffers and equals the eager calls."""
    from flash_attn_amd import kvcache_append_fp8, quantize_fp8
    Bn, H, D = 4, 8, 128
    g = torch.Generator().manual_seed(28)
    kd, vd = (torch.rand(Bn, HK, generator=g) + 0.05).to(DEV), (torch.rand(Bn, HK, generator=g) + 0.05).to(DEV)
    lens = torch.tensor([0, 3, 255, 256], dtype=torch.int32, device=DEV)
    q, k, v = [_rand((Bn, 1, h, D), torch.bfloat16, 29 + i).to(DEV) for i, h in enumerate((H, HK, HK))]
    kc, vc = torch.zeros(Bn, 512, HK, D, dtype=torch.uint8, device=DEV).view(FP8), torch.zeros(Bn, 512, HK, D, dtype=torch.uint8, device=DEV).view(FP8)

    def step(path):
        out = quantize_fp8(q, k, v, num_heads_k=HK, k_descale=kd, v_descale=vd, path=path)
        kvcache_append_fp8(kc, vc, k, v, lens, kd, vd)
        return out

    for path in (0, 1):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step(path)                                                     # warm-up: loads the library and the code objects outside the capture
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step(path)
        for r in range(2):
            for i, t in enumerate((q, k, v)):
                t.copy_(_rand(tuple(t.shape), torch.bfloat16, 40 + 3 * r + i, 1.0 + r).to(DEV))
            kc.view(torch.uint8).zero_(); vc.view(torch.uint8).zero_()
            graph.replay()
            torch.cuda.synchronize()
            got = [(y.clone(), ds.clone()) for y, ds in outs] + [kc.clone(), vc.clone()]
            kc.view(torch.uint8).zero_(); vc.view(torch.uint8).zero_()
            eager = step(path)
            torch.cuda.synchronize()
            _check(got[:3], [quant_ref(q, HK), quant_ref(k, HK, descale=kd.cpu()), quant_ref(v, HK, descale=vd.cpu())])
            for (y, ds), (ye, dse) in zip(got[:3], eager):
                assert torch.equal(y.view(torch.uint8), ye.view(torch.uint8)) and torch.equal(ds, dse)
            assert torch.equal(got[3].view(torch.uint8), kc.view(torch.uint8)) and torch.equal(got[4].view(torch.uint8), vc.view(torch.uint8))
            assert bool((kc.view(torch.uint8) != 0).any())
