"""sage_attn_qk_int8_pv_f16_masked -- the HAS_MASK instantiations of the attention kernel: a serial tile loop of their own, a
tile skip decided per wave, two load paths for the mask (a vector run of four, a scalar loop), fp32 logits t + mask and four
caller-given strides -- on the constructed int8 operands of tests/constructed_cases.py under STRUCTURED masks
(``mask_pattern``), against the fp64 softmax of exactly the keys each row keeps and the derived per-element bound (``bound``,
with its term for the additive form; tests/test_constructed_cases.py proves on the CPU that it is sound and has teeth).

Every element of o and of the base-2 LSE of every row that keeps a key is held to ratio <= 1 against the reference of its own
(batch, head) slice: no percentile, no fitted number.  Rows without a key exist only under ``row_switch`` (counted); the header
leaves them undefined, so what the kernel returns there is printed, not asserted.

The same mask VALUES are handed over in several layouts (contiguous; a window at an odd element offset of a poisoned parent
with an odd row pitch; a transposed parent, mask_strides[3] != 1: the scalar path; the unexpanded tensor with zero strides) and
must give the same BITS: vector path against scalar path."""
import ctypes

import pytest
import torch

import constructed_cases as C
from constructed_gpu_util import _Dev, _desc, _pinned

pytestmark = pytest.mark.gpu

_RECORD, _DEAD = {}, {}
_MASK_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}
_KIND = {torch.bool: 1, torch.uint8: 1, torch.float16: 2, torch.bfloat16: 3}


@pytest.fixture(scope="module")
def sa():
    assert torch.cuda.is_available()
    import sageattention_amd
    return sageattention_amd


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    if _RECORD:
        print("\nconstructed masks: largest |err| / bound over all elements of the rows that keep a key   [o, lse2]")
        for (what, fam, pv, D), (ro, rl) in sorted(_RECORD.items()):
            print(f"  {what:30s} {fam:13s} {pv:5s} D={D:<4d} {ro:6.3f} {rl:6.3f}")
    if _DEAD:
        print("\nrows without a key (row_switch; undefined by the header): what the kernel returned")
        for key, n in sorted(_DEAD.items()):
            print(f"  {key}: {n} rows")


def _record(what, fam, pv, D, ro, rl):
    a, b = _RECORD.get((what, fam, pv, D), (0.0, 0.0))
    _RECORD[(what, fam, pv, D)] = (max(a, ro), max(b, rl))


def _note_dead(o, lse, dead):
    """what the rows without a key hold, in words, for the summary table"""
    if not bool(dead.any()):
        return
    od, ld = o[dead].float(), lse[dead]
    what = ("o all 0" if bool((od == 0).all()) else "o all NaN" if bool(torch.isnan(od).all()) else
            "o finite" if bool(torch.isfinite(od).all()) else "o mixed non-finite")
    what += ", lse2 " + ("all -inf" if bool((ld == float("-inf")).all()) else "all NaN" if bool(torch.isnan(ld).all()) else
                         f"in [{float(ld.min()):.4g}, {float(ld.max()):.4g}]" if bool(torch.isfinite(ld).all()) else "mixed non-finite")
    _DEAD[what] = _DEAD.get(what, 0) + int(dead.sum())


class _MaskedCall:
    """one case's operands on the device, repeated over the Bm batch slices of the masks it will be called with"""

    def __init__(self, sa, c, pv, Bm=C.MASK_BM):
        from sageattention_amd import _lib as L
        self.L, self.c, self.pv, self.Bm = L, c, pv, Bm
        dev = _Dev(sa, c, pv)
        rep = lambda t: t.expand(Bm, *t.shape[1:]).contiguous()
        self.q8, self.k8, self.v, self.qs, self.ks = rep(dev.q8), rep(dev.k8), rep(dev.v), rep(dev.qs), rep(dev.ks)
        self.code = dev.code

    def run(self, mask, nw):
        """mask: a device [Bm,Hq,M,N] view of any strides -> (o, lse2) on the CPU, both NaN beforehand"""
        L, c = self.L, self.c
        M, N, D = c["M"], c["N"], c["D"]
        assert tuple(mask.shape) == (self.Bm, C.HQ, M, N) and mask.is_cuda
        o = torch.full((self.Bm, C.HQ, M, D), float("nan"), dtype=C.OUT_DTYPE[self.pv], device="cuda")
        lse = torch.full((self.Bm, C.HQ, M), float("nan"), device="cuda")
        st = (ctypes.c_int64 * 4)(*mask.stride())
        warpq = 128 if c["gran"] == "per_block" else 32
        with _pinned(nw):
            L.check(L.lib().sage_attn_qk_int8_pv_f16_masked(
                _desc(L, self.q8), _desc(L, self.k8), _desc(L, self.v), L.dtype_code(self.v.dtype), _desc(L, o),
                L.dtype_code(o.dtype), self.qs.data_ptr(), self.ks.data_ptr(), mask.data_ptr(), _KIND[mask.dtype], st,
                lse.data_ptr(), self.Bm, C.HQ, C.HK, M, N, D, self.code, 128, warpq, c["sm_scale"], 0,
                L.stream_ptr(o.device)), "masked")
            torch.cuda.synchronize()
        return o.cpu(), lse.cpu()


def _bits(t):
    return t.view(torch.int16) if t.dtype in (torch.float16, torch.bfloat16) else t


def _compact(mask):
    """the tensor an expanded view was expanded from: size 1 along every dimension of stride 0"""
    for d in range(mask.dim()):
        if mask.stride(d) == 0 and mask.shape[d] > 1:
            mask = mask.narrow(d, 0, 1)
    return mask.contiguous()


def _layouts(mask):
    """the same mask values in every layout -> [(name, device view, device parent, CPU copy of the parent)].
    window: [Bm,Hq,M+7,N+p] parent, p = 29 or 30 so that the row pitch is odd, the window at rows 3.., columns 11 or 12.. so
    that its element offset is odd too (an additive mask is then 2-byte aligned only); the rest of the parent holds "allowed"
    (bool) / NaN (additive).  transposed: a contiguous [Bm,Hq,N,M] parent viewed as [Bm,Hq,M,N]: mask_strides[3] = M.
    broadcast (expanded patterns only): the compact tensor with zero strides."""
    Bm, Hq, M, N = mask.shape
    dense = mask.contiguous()
    out = [("contiguous", dense.cuda(), None, None)]
    pitch = N + (29 if (N + 29) % 2 else 30)
    col = 11 if (3 * pitch + 11) % 2 else 12
    poison = True if mask.dtype == torch.bool else (1 if mask.dtype == torch.uint8 else float("nan"))
    parent = torch.full((Bm, Hq, M + 7, pitch), poison, dtype=mask.dtype)
    parent[:, :, 3:3 + M, col:col + N] = dense
    pd = parent.cuda()
    win = pd[:, :, 3:3 + M, col:col + N]
    assert win.stride(2) % 2 == 1 and win.storage_offset() % 2 == 1
    out.append(("window", win, pd, parent))
    tp = dense.transpose(2, 3).contiguous()
    td = tp.cuda()
    assert N == 1 or td.transpose(2, 3).stride(3) == M
    out.append(("transposed", td.transpose(2, 3), td, tp))
    if 0 in mask.stride():
        comp = _compact(mask)
        cd = comp.cuda()
        out.append(("broadcast", cd.expand(Bm, Hq, M, N), cd, comp))
    return out


def _check(call, d, o, lse, what, family, label, bad):
    """every element of the rows that keep a key against the bound; the rows without a key counted and noted"""
    c, pv = call.c, call.pv
    ro, rl, dead = C.mask_ratio_tensors(d, pv, o, lse)
    ro, rl = float(ro.max()), float(rl.max())
    _record(what, family, pv, c["D"], ro, rl)
    if not (ro <= 1.0 and rl <= 1.0):  # (a NaN ratio fails too)
        bad.append((label, what, ro, rl))
    _note_dead(o, lse, dead)
    return dead


def _expected_dead(name, M):
    return -(-(M - 5) // 16) if name == "row_switch" else 0


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", ["fp16", "bf16"])
@pytest.mark.parametrize("family", C.SUBSET_FAMILIES)
def test_masked_kernel_within_bound(sa, family, pv, D):
    """every case of subset_cases (all three granularities) under every pattern at M = 150, N = 456, contiguous masks with two
    batch slices (mask_strides[0] != 0), both geometries; bool masks as mask_kind 1, additive ones in V's type (kind 2 with
    fp16 V, kind 3 with bf16 V)"""
    bad = []
    masks = [(name, m, m.contiguous().cuda()) for name, m in C.mask_patterns(dtype=_MASK_DTYPE[pv])]
    for label, c in C.subset_cases(family, D, pv, C.GRANS):
        call = _MaskedCall(sa, c, pv)
        for name, m, md in masks:
            d = C.with_mask(c, m, name)
            for nw in (4, 8):
                o, lse = call.run(md, nw)
                dead = _check(call, d, o, lse, name, family, f"{label}-{name}-nw{nw}", bad)
                assert bool((dead.sum(-1) == _expected_dead(name, c["M"])).all()), (label, name)
    assert not bad, bad[:20]


def _uint8_of(mask):
    """a uint8 mask with the bits of the bool mask: False -> 0, True -> 1, 2, 128, 255 in turn"""
    _, _, r, n, _ = C._mask_index(mask.shape[2], mask.shape[3], mask.shape[0])
    vals = torch.tensor([1, 2, 128, 255], dtype=torch.uint8)[(r + n) % 4]
    return torch.where(mask, vals.expand_as(mask), torch.zeros((), dtype=torch.uint8))


def _same_bits_over_layouts(call, d, name, family, bad, also_uint8=False):
    """the mask of case ``d`` in every layout and both geometries: the contiguous result inside the bound, every other layout
    bit-identical to it, every parent unchanged"""
    mask = d["mask"]
    forms = _layouts(mask)
    if also_uint8:
        u8 = _uint8_of(mask)
        assert set(u8.unique().tolist()) <= {0, 1, 2, 128, 255} and torch.equal(u8 != 0, mask)
        forms += [(f"uint8-{nm}", v, p, cp) for nm, v, p, cp in _layouts(u8)]
    for nw in (4, 8):
        base = None
        for form, view, parent, parent_cpu in forms:
            o, lse = call.run(view, nw)
            if base is None:
                base = (o, lse)
                _check(call, d, o, lse, name, family, f"{name}-{form}-nw{nw}", bad)
            elif not (torch.equal(_bits(o), _bits(base[0])) and torch.equal(lse.view(torch.int32), base[1].view(torch.int32))):
                diff = int((_bits(o) != _bits(base[0])).sum()), int((lse.view(torch.int32) != base[1].view(torch.int32)).sum())
                bad.append((name, form, nw, "bits differ from the contiguous mask: (o elements, lse elements)", diff))
            if parent is not None and not torch.equal(_bits(parent.cpu()), _bits(parent_cpu)):
                bad.append((name, form, nw, "the mask's parent was written"))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", ["fp16", "bf16"])
def test_mask_layouts_give_the_same_bits(sa, pv, D):
    """scale_ladder (per_thread at head_dim 64, per_warp at 128) under every pattern, each in every layout; the bool patterns
    also as a uint8 mask holding {0, 1, 2, 128, 255} ("zero = masked"); the additive patterns in BOTH mask types, so that
    mask_kind 2 meets a bf16 V and mask_kind 3 an fp16 V (the C ABI takes the two independently)"""
    bad = []
    c = C.scale_ladder(D, C.SUBSET_N, False, "per_thread" if D == 64 else "per_warp")
    call = _MaskedCall(sa, c, pv)
    for name in C.BOOL_PATTERNS:
        _same_bits_over_layouts(call, C.with_mask(c, C.mask_pattern(name)), name, "scale_ladder", bad, also_uint8=True)
    for name in C.ADD_PATTERNS:
        for dt in (torch.float16, torch.bfloat16):
            tag = name if dt == _MASK_DTYPE[pv] else f"{name}/{'f16' if dt == torch.float16 else 'bf16'}"
            _same_bits_over_layouts(call, C.with_mask(c, C.mask_pattern(name, dtype=dt)), tag, "scale_ladder", bad)
    assert not bad, bad[:20]


@pytest.mark.parametrize("pv", ["fp16", "bf16"])
def test_a_mask_read_one_row_or_one_key_off_leaves_the_bound(sa, pv):
    """the teeth of the bound on the device: the window layout handed over one row down, or one key to the right (still inside
    its parent), is the mistake mask_next_row / mask_next_key of restate_mask64 made by the caller -- the kernel's result must
    leave the bound of the unshifted mask, for a bool and for an additive pattern"""
    c = C.scale_ladder(64, C.SUBSET_N, False, "per_thread")
    call = _MaskedCall(sa, c, pv)
    M, N = c["M"], c["N"]
    for name in ("late_first_key", "first_tile_off", "grid"):
        d = C.with_mask(c, C.mask_pattern(name, dtype=_MASK_DTYPE[pv]))
        _, win, parent, _ = _layouts(d["mask"])[1]
        r0, c0 = 3, win.storage_offset() % parent.stride(2)
        assert torch.equal(_bits(win), _bits(parent[:, :, r0:r0 + M, c0:c0 + N]))
        assert max(C.mask_ratios(d, pv, *call.run(win, 4))) <= 1.0
        for dr, dc in ((1, 0), (0, 1)):
            r = max(C.mask_ratios(d, pv, *call.run(parent[:, :, r0 + dr:r0 + dr + M, c0 + dc:c0 + dc + N], 4)))
            print(f"device teeth: {name:15s} {pv} shifted by ({dr} row, {dc} key): ratio {r:.3g}")
            assert r > 1.0, (name, dr, dc, r)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", ["fp16", "bf16"])
def test_small_shapes(sa, pv, D):
    """(M, N) = (1, 1), (5, 3), (33, 65), (128, 64): the case cut to size under one bool and one additive pattern built at that
    size.  N = 3 sends every run of four keys through the scalar path even at mask_strides[3] = 1, and 65 puts one key in a
    second tile; every layout, both geometries, all three granularities"""
    bad = []
    for gran in C.GRANS:
        c = C.scale_ladder(D, C.SUBSET_N, False, gran)
        for M, N in C.MASK_SMALL_SHAPES:
            d0 = C.cut_case(c, M, N)
            call = _MaskedCall(sa, d0, pv)
            for name, mask in C.mask_patterns(M, N, _MASK_DTYPE[pv], names=C.SMALL_PATTERNS):
                d = C.with_mask(d0, mask)
                assert not bool(C.no_key_rows(d).any())
                _same_bits_over_layouts(call, d, f"{M}x{N} {name}", "scale_ladder", bad, also_uint8=mask.dtype == torch.bool)
    assert not bad, bad[:20]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", ["fp16", "bf16"])
@pytest.mark.parametrize("backend", list(C.PUBLIC_BACKENDS))
def test_public_entry_with_masks(sa, backend, pv, D):
    """sageattn_qk_int8_pv_fp16_triton(q, k, v, attn_mask=..., smooth_k=False, return_lse=True) on the ``public_form`` cases:
    real Q and K from which BOTH quantizers of the backend return the case's int8 operands and scales (asserted here on the
    device, and on the CPU through the oracle's quantizers), so the fp64 reference and the bound of the case apply to the
    operator's result; the natural-log LSE under finish_bound with no q.km term.  Both backends reproduce the operands:
    "triton" with per-thread scales and sm_scale * log2e = 2^x in the kernel, "cuda" with per-block scales and that factor
    folded into Q.  key_padding is passed as [B,1,1,N] (the operator expands it), late_first_key as bool [B,Hq,M,N], neg_inf as
    an additive mask in q's dtype; both tensor layouts; B = 2, the batch slices of a mask differ."""
    dtype = _MASK_DTYPE[pv]
    bad = []
    gran = "per_thread" if backend == "triton" else "per_block_cuda"
    for label, d in C.public_cases(D, backend):
        q, k = (t.expand(C.MASK_BM, *t.shape[1:]).contiguous().cuda() for t in C.public_qk(d, dtype))
        v = C.v_of(d, pv).expand(C.MASK_BM, -1, -1, -1).contiguous().cuda()
        k8, ks, km = sa.core._prep_k(k, "HND", gran, False)
        q8, qs, _ = sa.core._quant_q(q, None, "HND", gran, d["sm_scale"], 32, False, C.HQ, C.HK)
        assert km is None and torch.equal(q8[0].cpu(), d["q8"][0]) and torch.equal(k8[0].cpu(), d["k8"][0]), label
        cgran = C.PUBLIC_BACKENDS[backend]
        assert torch.equal(C.O.expand_q_scale(qs.cpu(), d["M"], cgran)[:1], d["q_scale_rows"]), label
        assert torch.equal(C.O.expand_k_scale(ks.cpu(), d["N"], cgran)[:1], d["k_scale_cols"]), label
        for name, mask in C.mask_patterns(dtype=dtype, names=C.PUBLIC_PATTERNS):
            m = C.with_mask(d, mask)
            given = (_compact(mask) if name == "key_padding" else mask.contiguous()).cuda()
            assert name != "key_padding" or tuple(given.shape) == (C.MASK_BM, 1, 1, d["N"])
            ref = C.reference64(m, pv)
            o_b, l2_b = C.bound(m, pv)
            zero = torch.zeros_like(ref["lse2"])
            l_b = C.finish_bound(l2_b, ref["lse2"], zero)
            for layout in ("HND", "NHD"):
                tr = (lambda t: t) if layout == "HND" else (lambda t: t.transpose(1, 2).contiguous())
                o, lse = sa.sageattn_qk_int8_pv_fp16_triton(tr(q), tr(k), tr(v), tensor_layout=layout, quantization_backend=backend,
                                                            attn_mask=given, sm_scale=d["sm_scale"], smooth_k=False, return_lse=True)
                torch.cuda.synchronize()
                o = (o if layout == "HND" else o.transpose(1, 2)).cpu().double()
                lse = lse.cpu().double()
                assert tuple(o.shape) == tuple(ref["o"].shape) and tuple(lse.shape) == tuple(ref["lse2"].shape)
                fin = bool(torch.isfinite(o).all() and torch.isfinite(lse).all())
                ro = float(((o - ref["o"]).abs() / o_b).max()) if fin else float("inf")
                rl = float(((lse - C.finish_lse64(ref["lse2"], zero)).abs() / l_b).max()) if fin else float("inf")
                _record(f"public {backend} {name}", label, pv, D, ro, rl)
                if not (ro <= 1.0 and rl <= 1.0):
                    bad.append((label, name, layout, ro, rl))
    assert not bad, bad[:20]
