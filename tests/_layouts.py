"""Strided tensor layouts for the layout tests (test infrastructure only, CPU and GPU): a logical tensor placed into a poisoned arena under a named layout.

A kernel computes every address as base + (b * bs + row * rs + head * hs) * elem from a (batch, row, head) stride triple of ITS tensor; on contiguous
(B, S, H, D) tensors the triples of q / out / dout / dq coincide, and so do those of k / v / dk / dv, so a stride taken from the wrong tensor, a head stride
assumed to be D or a batch stride assumed to be S * rs changes nothing.  Here every tensor of a call gets a layout of its own, and everything around it is poison:

  input arenas     every element outside the view is NaN: a read through a wrong stride, past the last row or past D lands in NaN (or in other data) and shows
                   in the result;
  output arenas    every element, view included, holds SENTINEL (an int16 bit pattern, a finite value in bf16 and fp16): a store outside the view changes a
                   sentinel, a missed store inside the view leaves one.

Every arena has >= PAD_ROWS rows' worth of poison before and after the buffer, so an over-read or over-write of a tile lands in the arena and is reported
instead of touching unmapped memory.  The arena starts 16 bytes into its allocation: every base is 16-byte aligned and the contiguous one is NOT 32-byte aligned.

Layouts of a (B, S, H, D) tensor -- and of a packed (T, H, D) one, and of a paged cache (pages, page, Hk, D), where they apply:
  bshd         contiguous
  bhsd         transpose(1, 2) of (B, H, S, D): rs = D, hs = S * D                (packed: transpose(0, 1) of (H, T, D); paged: the page-internal (Hk, page, D) order)
  sbhd         transpose(0, 1) of (S, B, H, D): bs = H * D, rs = B * H * D        (packed: column 1 of a (T, 2, H, D) buffer, rs = 2 * H * D)
  fused_proj   column slices of ONE (B, S, sum(H_i) * D) arena (place_fused): rs = sum(H_i) * D, hs = D, bases sum(H_j, j < i) * D apart
  padded_head  [..., :D] of (B, S, H, D + 16 bytes): heads 16 bytes further apart, poison between them
  row_skip     [:, 1::2] of (B, 2 S + 1, H, D)                                     (packed: [1::2] of (2 T + 1, H, D))
  bcast_b      expand of a (1, S, H, D) buffer over the batch: bs = 0 (inputs only)
  page_skip    every second page of a pool of 2 * pages + 1 (the dimension-0 form of row_skip)
"""
import torch

PAD_ROWS = 128
SENTINEL = 0x5A5A   # int16; bf16 1.5e16, fp16 203.25: finite in both, and nothing an attention of unit-scale inputs returns
LAYOUTS = ("bshd", "bhsd", "sbhd", "fused_proj", "padded_head", "row_skip", "bcast_b", "page_skip")
_NAN_BITS = {torch.bfloat16: (torch.int16, 0x7FC0), torch.float16: (torch.int16, 0x7E00), torch.float32: (torch.int32, 0x7FC00000), torch.float64: (torch.int64, 0x7FF8000000000000),
             torch.float8_e4m3fn: (torch.uint8, 0x7F)}


def _chunk(dtype):   # elements per 16 bytes
    return 16 // torch.empty((), dtype=dtype).element_size()


def _physical(layout, shape, dtype):
    """(physical buffer shape, buffer -> view) of a logical shape under a layout."""
    n = len(shape)
    if layout == "bshd":
        return tuple(shape), lambda b: b
    if layout == "padded_head":
        return tuple(shape[:-1]) + (shape[-1] + _chunk(dtype),), lambda b: b[..., :shape[-1]]
    if layout == "page_skip":
        return (2 * shape[0] + 1,) + tuple(shape[1:]), lambda b: b[1::2]
    if n == 4:
        B, S, H, D = shape
        if layout == "bhsd":
            return (B, H, S, D), lambda b: b.transpose(1, 2)
        if layout == "sbhd":
            return (S, B, H, D), lambda b: b.transpose(0, 1)
        if layout == "row_skip":
            return (B, 2 * S + 1, H, D), lambda b: b[:, 1::2]
        if layout == "bcast_b":
            return (1, S, H, D), lambda b: b.expand(B, S, H, D)
    if n == 3:
        T, H, D = shape
        if layout == "bhsd":
            return (H, T, D), lambda b: b.transpose(0, 1)
        if layout == "sbhd":
            return (T, 2, H, D), lambda b: b[:, 1]
        if layout == "row_skip":
            return (2 * T + 1, H, D), lambda b: b[1::2]
    raise ValueError(f"layout {layout} of a {n}-D tensor")


class Arena:
    """One allocation: .flat (the arena, poison margins included), .views (the logical tensors), .kind ('input' | 'output')."""

    def __init__(self, phys_shape, row_elems, dtype, kind, device):
        c = _chunk(dtype)
        n = 1
        for s in phys_shape:
            n *= s
        margin = -(-PAD_ROWS * max(row_elems, 1) // (2 * c)) * 2 * c    # a multiple of 32 bytes: the buffer keeps the arena's alignment
        self.kind, self.dtype, self.margin, self.views = kind, dtype, margin, []
        self._alloc = torch.empty(c + 2 * margin + n, dtype=dtype, device=device)
        self.flat = self._alloc[c:]
        it, nan = _NAN_BITS[dtype]
        self.bits().fill_(SENTINEL if kind == "output" else nan)
        self.buf = self.flat[margin:margin + n].view(phys_shape)
        self._snapshot = None

    def bits(self):
        return self.flat.view(_NAN_BITS[self.dtype][0])

    def add(self, view, data=None):
        assert view.untyped_storage().data_ptr() == self._alloc.untyped_storage().data_ptr()
        if data is not None:
            if 0 in view.stride():   # an expanded view: written once, through the buffer it expands
                idx = tuple(slice(0, 1) if st == 0 and n > 1 else slice(None) for st, n in zip(view.stride(), view.shape))
                view[idx].copy_(data[idx])
            else:
                view.copy_(data)
        self.views.append(view)
        return view

    def view_mask(self):
        """bool per element of .flat: True where some view has an element."""
        mask = torch.zeros(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        index = torch.arange(self.flat.numel(), device=self.flat.device)
        for v in self.views:
            mask[index.as_strided(v.shape, v.stride(), v.storage_offset() - self.flat.storage_offset()).reshape(-1)] = True
        return mask

    def freeze(self):
        """Remember the arena's bits: unchanged() compares against them."""
        self._snapshot = self.bits().clone()

    def unchanged(self):
        return torch.equal(self.bits(), self._snapshot)

    def outside_intact(self):
        """An output arena: every element outside the views still holds the sentinel.  An input arena: every element outside the views still holds the NaN."""
        want = SENTINEL if self.kind == "output" else _NAN_BITS[self.dtype][1]
        return bool((self.bits()[~self.view_mask()] == want).all())

    def outside_unchanged(self):
        """A tensor a call reads AND writes (an appended cache): everything outside the views is bit-identical to the frozen arena."""
        m = ~self.view_mask()
        return torch.equal(self.bits()[m], self._snapshot[m])


def place(layout, data=None, shape=None, dtype=None, kind="input", device=None):
    """A logical tensor (data, or for an output its shape and dtype) under a layout -> (arena, view).  bcast_b keeps batch entry 0 of data."""
    if data is not None:
        shape, dtype, device = tuple(data.shape), data.dtype, data.device if device is None else device
        data = data.to(device)
    assert layout != "fused_proj", "place_fused"
    assert not (kind == "output" and layout == "bcast_b")
    phys, to_view = _physical(layout, tuple(shape), dtype)
    probe = to_view(torch.empty(phys, dtype=dtype, device="meta"))
    a = Arena(phys, abs(probe.stride(-3)) if len(shape) >= 3 else shape[-1], dtype, kind, device)
    view = a.add(to_view(a.buf), data)
    assert tuple(view.shape) == tuple(shape)
    if kind == "input":
        a.freeze()
    return a, view


def place_fused(datas=None, shapes=None, dtype=None, kind="input", device=None, spare_heads=0):
    """Several (B, S_i, H_i, D) -- or packed (T_i, H_i, D) -- tensors as column slices of ONE (B, max S, sum(H_i * D_i)) arena: q, k and v of a fused projection, or
    dq, dk and dv of a packed gradient (spare_heads more heads of poison columns at the end: the slices of a projection this call does not take).  A tensor with fewer rows than the arena uses the first S_i; the rest of its columns is poison.  -> (arena, [views])."""
    if datas is not None:
        shapes, dtype, device = [tuple(d.shape) for d in datas], datas[0].dtype, datas[0].device if device is None else device
    lead = len(shapes[0]) - 2                       # 2 leading dimensions (B, S) or 1 (T)
    assert all(s[:lead - 1] == shapes[0][:lead - 1] for s in shapes)
    rows = max(s[lead - 1] for s in shapes)
    width = sum(s[-2] * s[-1] for s in shapes) + spare_heads * shapes[0][-1]   # (each tensor keeps its own head dim: v of the (192, 128) pair is narrower)
    a = Arena(tuple(shapes[0][:lead - 1]) + (rows, width), width, dtype, kind, device)
    views, col = [], 0
    for i, s in enumerate(shapes):
        v = a.buf[..., :s[lead - 1], col:col + s[-2] * s[-1]].unflatten(-1, (s[-2], s[-1]))
        views.append(a.add(v, None if datas is None else datas[i].to(device)))
        col += s[-2] * s[-1]
    if kind == "input":
        a.freeze()
    return a, views


# ---- assignments: role -> layout -----------------------------------------------------------------------------------------------------------------
# ("fused_proj" names a group: the roles that carry the same group tag share one arena)
ATTN_ROLES = ("q", "k", "v", "out", "dout", "dq", "dk", "dv")
CACHE_ROLES = ("q", "kcache", "vcache", "knew", "vnew", "out")
OUTPUT_ROLES = ("out", "dq", "dk", "dv")
FUSED_GROUPS = {"q": "qkv", "k": "qkv", "v": "qkv", "knew": "qkv", "vnew": "qkv", "dq": "dqkv", "dk": "dqkv", "dv": "dqkv"}
ASSIGNMENTS = {
    # A1 "as callers do": q / k / v column slices of one fused projection, out through a (B, H, S, D) buffer, dout in Megatron's (S, B, H, D), gradients into one packed arena
    "A1": dict(q="fused_proj", k="fused_proj", v="fused_proj", out="bhsd", dout="sbhd", dq="fused_proj", dk="fused_proj", dv="fused_proj",
               kcache="padded_head", vcache="row_skip", knew="fused_proj", vnew="fused_proj"),
    # A2 / A3 "all different": within a call no two tensors share a (bs, rs, hs) triple
    "A2": dict(q="bhsd", k="sbhd", v="padded_head", out="row_skip", dout="padded_head", dq="sbhd", dk="row_skip", dv="bhsd",
               kcache="sbhd", vcache="padded_head", knew="row_skip", vnew="sbhd"),
    "A3": dict(q="row_skip", k="padded_head", v="bhsd", out="sbhd", dout="bhsd", dq="padded_head", dk="sbhd", dv="row_skip",
               kcache="row_skip", vcache="bhsd", knew="bhsd", vnew="padded_head"),
    # A4 (forward and cache only): k / v expanded over the batch
    "A4": dict(q="sbhd", k="bcast_b", v="bcast_b", out="padded_head", kcache="bcast_b", vcache="bcast_b", knew="row_skip", vnew="bhsd"),
}
# paged caches (pages, page, Hk, D): the pool forms of the same assignments (bhsd = the page-internal (Hk, page, D) order)
PAGED = {"A1": dict(kcache="page_skip", vcache="bhsd"), "A2": dict(kcache="bhsd", vcache="padded_head"), "A3": dict(kcache="padded_head", vcache="page_skip"),
         "A4": dict(kcache="page_skip", vcache="padded_head")}


def place_call(assignment, inputs, outputs, dtype=None, device=None, paged=False):
    """inputs {role: data}, outputs {role: shape} under an assignment -> ({role: view}, [arenas]).  Roles of a fused group present in the call share an arena."""
    table = dict(ASSIGNMENTS[assignment], **(PAGED[assignment] if paged else {}))
    views, arenas = {}, []
    for roles, kind in ((inputs, "input"), (outputs, "output")):
        groups = {}
        for role, x in roles.items():
            if x is None:
                views[role] = None
            elif table[role] == "fused_proj":
                groups.setdefault(FUSED_GROUPS[role], []).append(role)
            elif kind == "input":
                a, views[role] = place(table[role], data=x, device=device)
                arenas.append(a)
            else:
                a, views[role] = place(table[role], shape=x, dtype=dtype, kind="output", device=device)
                arenas.append(a)
        for members in groups.values():
            if kind == "input":
                a, vs = place_fused(datas=[roles[m] for m in members], device=device, spare_heads=2 if len(members) == 1 else 0)
            else:
                a, vs = place_fused(shapes=[roles[m] for m in members], dtype=dtype, kind="output", device=device, spare_heads=2 if len(members) == 1 else 0)
            arenas.append(a)
            views.update(zip(members, vs))
    return views, arenas


def triple(t):
    """(bs, rs, hs) of a 4-D tensor, (rs, hs) of a packed one."""
    return tuple(t.stride()[:-1])


# ---- the case list of tests/test_layout_matrix_gpu.py: census recipes by id ------------------------------------------------------------------------
def _ids(pattern, **axes):
    out = [pattern]
    for name, values in axes.items():
        out = [p.replace("{" + name + "}", str(v)) for p in out for v in values]
    return out


FC = ("full", "causal")
CASE_IDS = (
    # lock-step forward at 4 / 8 waves and ping-pong; its window row, dropout, ALiBi + softcap, fp16 twin (fa_fwd.hip)
    _ids("fwd-bf16-d{d}-nw{nw}-plain-{m}", d=(64, 128), nw=(4, 8), m=FC) + _ids("fwd-bf16-d{d}-pingpong-plain-{m}", d=(64, 128), m=FC)
    + ["fwd-bf16-d128-nw4-plain-local", "fwd-bf16-d128-nw4-drop-causal", "fwd-bf16-d128-nw8-all-full", "fwd-f16-d128-nw4-plain-causal"]
    # head dim 256, trimmed head dims 96 / 32 (and 192, the third trimmed pitch), forward and backward
    + _ids("d256-bf16-plain-{m}", m=FC) + _ids("d{d}-bf16-{side}-plain-{m}", d=(32, 96), side=("fwd", "bwd"), m=FC) + ["d192-bf16-plain-causal"]
    # pipelined forward: 4 / 8 waves x schedules 0 / 3 (fa_fwd_il.hip)
    + _ids("fwd_il-bf16-d128-nw{nw}-sched{s}-{m}", nw=(4, 8), s=(0, 3), m=FC)
    + ["fwd_il-bf16-d64-nw4-sched3-causal", "fwd_il-bf16-d64-nw8-sched0-full", "fwd_il-bf16-d128-nw4-sched3-local", "fwd_il-f16-d128-nw4-sched3-causal"]
    # 64-rows-per-wave forward: dense, packed, paged prefill (fa_fwd_w64.hip)
    + _ids("fwd_w64-bf16-d{d}-{k}-{m}", d=(64, 128), k=("dense", "varlen", "paged"), m=FC)
    + ["fwd_w64-bf16-d128-general-local", "fwd_w64-bf16-d128-drop-causal", "fwd_w64-bf16-d128-alibi-causal", "fwd_w64-bf16-d128-cap-full", "fwd_w64-f16-d128-dense-causal"]
    # (192, 128) forward and backward (fa_fwd_dv.hip), MLA contiguous / paged / split (fa_fwd_mla.hip)
    + _ids("dv192_128-bf16-{m}", m=FC + ("local",)) + ["dv192_128-f16-causal"]
    + _ids("mla-bf16-{m}", m=FC + ("local", "paged-causal", "split")) + ["mla-f16-causal"]
    # split keys + combine at every pitch, paged; head packing off and cache_batch_idx are derived rows (below)
    + _ids("split-bf16-d{d}", d=(32, 64, 96, 128, 192, 256)) + ["split-bf16-d128-paged", "split-bf16-d128+nopack", "split-bf16-d128+batch_idx", "split-f16-d128"]
    + ["kv_append", "rotary-bf16", "rotary-f16"]
    # both fp8 forwards
    + _ids("fp8-d{d}-{m}", d=(64, 128), m=FC) + ["fp8-d128-local"] + _ids("fp8kv-d{d}-ring4-{m}", d=(64, 128), m=FC)
    + ["fp8kv-d128-ring4-local", "fp8kv-d128-ring4-paged-causal", "fp8kv-d128-ring2-causal", "fp8kv-d128-ring3-causal"]
    # backward pair: delta, dQ at 4 / 8 waves, dK/dV at 8 waves (fa_bwd.hip)
    + _ids("bwd-bf16-d{d}-dq{nw}-plain-{m}", d=(64, 128), nw=(4, 8), m=FC)
    + ["bwd-bf16-d128-dq4-plain-local", "bwd-bf16-d128-dq4-drop-causal", "bwd-bf16-d128-dq8-all-full", "bwd-f16-d128-dq4-plain-causal"]
    # 64-per-wave dQ (delta fused or not) and dK/dV (fa_bwd_w64.hip, fa_bwd_dkdv_w64.hip)
    + _ids("bwd_w64-bf16-d{d}-fuse{f}-plain-{m}", d=(64, 128), f=(0, 1), m=FC)
    + ["bwd_w64-bf16-d128-fuse1-plain-local", "bwd_w64-bf16-d128-fuse1-alibi-causal", "bwd_w64-bf16-d128-fuse1-cap-full", "bwd_w64-bf16-d128-fuse1-drop-causal",
       "bwd_w64-f16-d128-fuse1-plain-causal"]
    # the fused launch, the chunked launch, the group split with gsum, varlen_bwd with and without its work lists
    + _ids("bwd_fused-bf16-d{d}-{m}", d=(64, 128), m=FC) + _ids("bwd_c5-bf16-d{d}-{m}", d=(64, 128), m=FC) + ["bwd_c5-f16-d128-causal"]
    + _ids("bwd_gsum-bf16-{m}", m=FC) + ["bwd-bf16-d128-dq4-plain-causal+varlen", "bwd-bf16-d128-dq4-plain-causal+varlen_lists"]
)
# rows derived from a census row ("<id>+<variant>"): the same call with one more argument the census has no row for
VARLEN_LISTS = [37] * 7 + [512] + [37] * 8   # (tests/test_kernel_census_gpu.py _run_schedule: uneven enough for the work lists)
DERIVED = {"nopack": dict(knobs={"FA_PACK_GQA": 0}), "batch_idx": dict(batch_idx=True), "varlen": dict(varlen=True), "varlen_lists": dict(varlen=True, lens=VARLEN_LISTS)}
STRIDELESS = ("fa_varlen_schedule_kernel", "fa_set_rng_kernel")   # the two kernels that take no tensor stride


def select_cases(recipes):
    """The rows of CASE_IDS, in that order: census rows by id, derived rows as copies with the variant's fields laid over them."""
    by_id = {r["id"]: r for r in recipes}
    rows = []
    for cid in CASE_IDS:
        base, _, variant = cid.partition("+")
        row = dict(by_id[base], id=cid)
        if variant:
            extra = DERIVED[variant]
            row.update({k: v for k, v in extra.items() if k != "knobs"}, knobs=dict(row["knobs"], **extra.get("knobs", {})))
        rows.append(row)
    return rows


_HEAD_DIMS = (32, 64, 96, 128, 192, 256, 512, 576)


def pitch(key):
    """(family, leading head-dim template arguments) of a census key: the head-dim pitch a kernel is built for."""
    family, _, args = key
    dims = []
    for a in args:
        if type(a) is not int or a not in _HEAD_DIMS:
            break
        dims.append(a)
    return (family, tuple(dims))


def assignments_of(row):
    """A1 - A3 everywhere; A4 (k / v expanded over the batch) on forward and cache rows -- not where k / v are also written (the append), have gradients
    (a backward row) or are indexed per entry of a packed batch."""
    bwd = any(k[0].startswith("fa_bwd") for k in row["keys"])
    packed = row.get("varlen", False)
    no_a4 = bwd or packed or row["kind"] in ("append", "rotary")
    return ("A1", "A2", "A3") + (() if no_a4 else ("A4",))
