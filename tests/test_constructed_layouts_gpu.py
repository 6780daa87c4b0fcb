"""Batch, head, sequence and tile ADDRESSING of the attention kernels on the constructed int8 operands of
tests/constructed_cases.py: one call that holds several DIFFERENT cases -- stacked over 2 batches x 2 KV heads (``stack``, GQA
group 2: four query heads), packed as sequences of different lengths (``pack``), or laid out tile-major (``tile_major``) -- and
top-left causal calls with M != N (``cut_case``).  Every slice of a result is held to the fp64 reference and the derived
per-element bound of the case that was put there: every element of o and of the LSE at ratio <= 1, no percentile, no fitted
number.  tests/test_constructed_cases.py proves on the CPU that the bounds are sound for these forms and that each of the ten
addressing mistakes of ``LAYOUT_MISTAKES`` (the K scales of KV head 0, the K / V of batch 0, the interleaved workgroup id
decoded batch-major, the workspace slot of head 0, cu_seqlens one row off, the scale rows of the previous sequence or at the
wrong row pitch, a bottom-right diagonal, tile-major scales or tiles read with dense strides) leaves them.

The slots of a stack differ where it matters: a scale ladder, an ascending and a descending step-40 ramp and a hot last key,
their scales moved apart by powers of two (``rebalance``), the two query heads of every slot different (``distinct_heads``).

Every entry point is called through the C ABI on operands copied from the CPU builders; o, lse and workspaces are NaN before
every call; poison as in tests/test_constructed_subsets_gpu.py beyond a batch's length, around packed windows and between
tiles."""
import ctypes

import pytest
import torch

import constructed_cases as C
import splitkv_causal_util as CU
from constructed_gpu_util import GRAN_CODE, _desc, _pinned, _StackDev, fp8_kernel_order

pytestmark = pytest.mark.gpu

_RECORD = {}
NEG_INF = float("-inf")
NAN = float("nan")
GRANS2 = ("per_warp", "per_thread")


@pytest.fixture(scope="module")
def sa():
    assert torch.cuda.is_available()
    import sageattention_amd
    return sageattention_amd


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    if _RECORD:
        print("\nconstructed layouts: largest |err| / bound over all elements   [o, lse]")
        for (what, fam, pv, D), (ro, rl) in sorted(_RECORD.items()):
            print(f"  {what:20s} {fam:13s} {pv:5s} D={D:<4d} {ro:6.3f} {rl:6.3f}")


def _record(what, fam, pv, D, ro, rl):
    a, b = _RECORD.get((what, fam, pv, D), (0.0, 0.0))
    _RECORD[(what, fam, pv, D)] = (max(a, ro), max(b, rl))


def _hold_stack(st, pv, o, lse, what, label, bad, sub=None):
    """every slot of a stacked result against its own case (``sub(case, b)``: the case batch b's slots are held to)"""
    for b in range(st["Bs"]):
        for hk in range(st["Hks"]):
            own = st["grid"][b][hk]
            c = own if sub is None else sub(own, b)
            hs = C.slot_heads(hk)
            ro, rl = C.ratios(c, pv, o[b:b + 1, hs], lse[b:b + 1, hs])
            _record(what, own["family"], pv, st["D"], ro, rl)
            if not (ro <= 1.0 and rl <= 1.0):
                bad.append((label, what, b, hk, own["family"], ro, rl))


# ---- a. stacked, every kernel family ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
def test_stacked_dense(sa, pv, D):
    """sage_attn_qk_int8_pv_{f16,f8}: 4 and 8 waves, non-causal (M = 150) and causal (M = N = 456), every granularity"""
    bad = []
    for gran in C.GRANS:
        for causal in (False, True):
            st = C.stack_slots(D, 456, causal, gran)
            dev = _StackDev(sa, st, pv)
            for nw in (4, 8):
                o, lse = dev.run("", causal, nw=nw)
                _hold_stack(st, pv, o, lse, "dense", f"{gran}-{'causal' if causal else 'full'}-nw{nw}", bad)
    assert not bad, bad[:20]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
def test_stacked_kv_lens(sa, pv, D):
    """the _kvlen twins with kv_lens (257, 456) and (456, 64), poison beyond each length: batch b against
    subcase(slot, length = len_b).  The workgroup id of these kernels alternates the batches inside a head."""
    bad = []
    for gran in C.GRANS:
        for causal in (False, True):
            st = C.stack_slots(D, 456, causal, gran)
            for lens in C.STACK_KV_LENS:
                dev = _StackDev(sa, st, pv, lens)
                for nw in (4, 8):
                    o, lse = dev.run("kvlen", causal, kv_lens=True, nw=nw)
                    _hold_stack(st, pv, o, lse, "kvlen", f"{gran}-{'causal' if causal else 'full'}-{lens}-nw{nw}", bad,
                                sub=lambda own, b: C.cached_subcase(own, None, lens[b]))
    assert not bad, bad[:20]


SPARSE_MAPS = ("mixed", "alternate")


def _stack_map(st):
    """bool [Bs,Hq,2,ntk]: (b, h) takes head h % 2 of SPARSE_MAPS[(b + h) % 2] -- neighbouring heads of a batch differ, and so
    do rows b * Hq + h and h * Bs + b for some (b, h) -> (map, tile lists [b][h][qb])"""
    ntk = (st["N"] + 63) // 64
    bm = torch.zeros(st["Bs"], st["Hq"], 2, ntk, dtype=torch.bool)
    tiles = [[C.SUBSET_MAPS[SPARSE_MAPS[(b + h) % 2]][h % 2] for h in range(st["Hq"])] for b in range(st["Bs"])]
    for b in range(st["Bs"]):
        for h in range(st["Hq"]):
            for qb in range(2):
                bm[b, h, qb, tiles[b][h][qb]] = True
    rows = bm.view(-1, 2, ntk)
    assert all(not torch.equal(bm[b, h], bm[b, h + 1]) for b in range(st["Bs"]) for h in range(st["Hq"] - 1))
    assert any(not torch.equal(rows[b * st["Hq"] + h], rows[h * st["Bs"] + b]) for b in range(st["Bs"]) for h in range(st["Hq"]))
    return bm, tiles


def _hold_map(st, pv, o, lse, tiles, lens, what, label, bad):
    """every (b, h, q-block) of a block-sparse result against the subcase of its own tile list clipped to the batch's length"""
    M, N = st["M"], st["N"]
    for b in range(st["Bs"]):
        length = N if lens is None else lens[b]
        for h in range(st["Hq"]):
            own, hs, hl = st["grid"][b][h // C.HQ], C.slot_heads(h // C.HQ), h % C.HQ
            for qb in range(2):
                rs = slice(128 * qb, min(128 * qb + 128, M))
                ts = [t for t in tiles[b][h][qb] if 64 * t < length]
                if not ts:  # no tile below the length: the convention of empty q-blocks
                    if not (torch.equal(o[b, h, rs], torch.zeros_like(o[b, h, rs])) and bool((lse[b, h, rs] == NEG_INF).all())):
                        bad.append((label, what, b, h, qb, "empty q-block is not 0 / -inf"))
                    continue
                d = C.cached_subcase(own, ts, None if lens is None else length)
                ro, rl = C.ratio_tensors(d, pv, o[b:b + 1, hs], lse[b:b + 1, hs])
                ro, rl = float(ro[0, hl, rs].max()), float(rl[0, hl, rs].max())
                _record(what, own["family"], pv, st["D"], ro, rl)
                if not (ro <= 1.0 and rl <= 1.0):
                    bad.append((label, what, b, h, qb, ts, ro, rl))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
def test_stacked_block_sparse(sa, pv, D):
    """the _blocksparse and _blocksparse_kvlen entry points under a map that differs per (b, h) (two of SUBSET_MAPS assigned
    alternately): the list row of a workgroup is that of its own (b, h) whichever way its id is numbered"""
    bad = []
    for gran in C.GRANS:
        st = C.stack_slots(D, 456, False, gran)
        bm, tiles = _stack_map(st)
        lists = sa.block_sparse_plan(bm.cuda(), st["M"], st["N"], B=st["Bs"], Hq=st["Hq"]).lists
        o, lse = _StackDev(sa, st, pv).run("blocksparse", lists=lists)
        _hold_map(st, pv, o, lse, tiles, None, "sparse", gran, bad)
        for lens in C.STACK_KV_LENS:
            o, lse = _StackDev(sa, st, pv, lens).run("blocksparse_kvlen", lists=lists, kv_lens=True)
            _hold_map(st, pv, o, lse, tiles, lens, "sparse+kvlen", f"{gran}-{lens}", bad)
    assert not bad, bad[:20]


# (granularity, Q / output dtype) per PV type, as tests/test_constructed_subsets_gpu.py pairs them
SPLIT_COMBOS = {"fp16": (("per_warp", torch.float16), ("per_thread", torch.float16)),
                "bf16": (("per_warp", torch.bfloat16), ("per_thread", torch.bfloat16)),
                "fp8": (("per_warp", torch.float16), ("per_thread", torch.bfloat16))}
SPLIT_SHAPES = ((456, (2, 3)), (512, (4, 8)))
SPLIT_LENS = (None, (257, 512))


class _StackSplit:
    """sage_attn_fusedq_pv_{f16,f8}_splitkv[_causal] on an anchored stack; km differs per slot (constructed_cases.stack_km)"""

    def __init__(self, sa, st, pv, dtype, lens):
        from sageattention_amd import _lib as L
        assert st["anchored"]
        self.L, self.st, self.pv, self.given = L, st, pv, lens
        self.dev = _StackDev(sa, st, pv, lens)
        self.lens = self.dev.lens
        self.q = torch.cat([torch.cat([C.q_real(c, dtype) for c in row], dim=1) for row in st["grid"]], dim=0).cuda()
        self.km_cpu = C.stack_km(st)
        self.km = self.km_cpu.to(dtype).cuda()
        assert torch.equal(self.km.float().cpu(), self.km_cpu)
        self.kv_lens = None if lens is None else torch.tensor(list(lens), dtype=torch.int32, device="cuda")  # as given: clamped there

    def qkm(self, b, hk):
        return C.split_qkm(self.st["grid"][b][hk], self.km_cpu[b:b + 1, hk:hk + 1])

    def run(self, S, q_fold=None):
        """-> (o, lse, o_parts fp32 [S,B,Hq,M,D], lse2_parts fp32 [S,B,Hq,M]) on the CPU"""
        L, st, dev = self.L, self.st, self.dev
        B, Hq, Hk, M, N, D = dev.B, dev.Hq, dev.Hk, st["M"], st["N"], st["D"]
        o = torch.full((B, Hq, M, D), NAN, dtype=self.q.dtype, device="cuda")
        lse = torch.full((B, Hq, M), NAN, device="cuda")
        nbytes = L.lib().sage_splitkv_workspace_bytes(B, Hq, M, D, S)
        assert nbytes == S * B * Hq * M * (D + 1) * 4
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")  # every fp32 word a NaN
        shape = (B, Hq, Hk, M, N, D, GRAN_CODE[st["gran"]], 32, st["sm_scale"])
        tail = (None if self.kv_lens is None else self.kv_lens.data_ptr(), S) + (() if q_fold is None else (q_fold,)) + \
               (ws.data_ptr(), nbytes, L.stream_ptr(o.device))
        q, k = (_desc(L, self.q), L.dtype_code(self.q.dtype)), _desc(L, dev.k8)
        out = (_desc(L, o), L.dtype_code(o.dtype), dev.ks.data_ptr(), self.km.data_ptr())
        sym = f"sage_attn_fusedq_pv_{'f8' if self.pv == 'fp8' else 'f16'}_splitkv" + ("" if q_fold is None else "_causal")
        if self.pv == "fp8":
            s = getattr(L.lib(), sym)(*q, k, _desc(L, dev.v), *out, dev.v_scale.data_ptr(), None, lse.data_ptr(), *shape, *tail)
        else:
            s = getattr(L.lib(), sym)(*q, k, _desc(L, dev.v), L.dtype_code(dev.v.dtype), *out, None, lse.data_ptr(), *shape, *tail)
        L.check(s, sym)
        torch.cuda.synchronize()
        f = ws.view(torch.float32).cpu()
        n_o = S * B * Hq * M * D
        return o.cpu(), lse.cpu(), f[:n_o].view(S, B, Hq, M, D), f[n_o:].view(S, B, Hq, M)


def _hold_split(call, S, label, bad):
    """every slot: the partials in the workspace slots [S,B,Hq,M,(D)] of its own (b, h) under ``bound`` of the split's subcase,
    the slots of empty splits still NaN, the merged o and the finished LSE under merged_bound / finish_bound"""
    st, pv = call.st, call.pv
    o, lse, o_parts, l2_parts = call.run(S)
    if torch.isnan(o.float()).any() or torch.isnan(lse).any():
        bad.append((label, S, "NaN in the result"))
    for b, n in enumerate(call.lens):
        for hk in range(st["Hks"]):
            own, hs, qkm = st["grid"][b][hk], C.slot_heads(hk), call.qkm(b, hk)
            cn = own if n == own["N"] else C.cached_subcase(own, None, n)
            subs = C.split_subcases(cn, S)
            for s in range(S):
                po, pl = o_parts[s, b:b + 1, hs].double(), l2_parts[s, b:b + 1, hs].double()
                if s >= len(subs):
                    if not (torch.isnan(po).all() and torch.isnan(pl).all()):
                        bad.append((label, S, b, hk, s, "slot of an empty split written"))
                    continue
                ref = C.reference64(subs[s], pv)
                o_b, l_b = C.bound(subs[s], pv, out_ulps=0)
                ok = bool(torch.isfinite(po).all() and torch.isfinite(pl).all())
                ro = float(((po - ref["o"]).abs() / o_b).max()) if ok else float("inf")
                rl = float(((pl - ref["lse2"]).abs() / l_b).max()) if ok else float("inf")
                _record("splitkv part", own["family"], pv, st["D"], ro, rl)
                if not (ro <= 1.0 and rl <= 1.0):
                    bad.append((label, S, b, hk, s, "partial", ro, rl))
            ro, rl = C.merged_ratios(cn, pv, S, o[b:b + 1, hs], lse[b:b + 1, hs], qkm, o.dtype)
            _record("splitkv", own["family"], pv, st["D"], ro, rl)
            if not (ro <= 1.0 and rl <= 1.0):
                bad.append((label, S, b, hk, "merged", ro, rl))


@pytest.mark.parametrize("N,splits", SPLIT_SHAPES, ids=[f"N{n}" for n, _ in SPLIT_SHAPES])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
def test_stacked_split_kv(sa, pv, D, N, splits):
    """sage_attn_fusedq_pv_{f16,f8}_splitkv on the anchored stack (the fused quantizer returns the chosen q8 and 2^e exactly), a
    non-zero km per slot, kv_lens NULL and (257, 512) (clamped to N = 456 by the kernel), S in (2, 3) at N = 456 and (4, 8) at
    N = 512: the workspace slot of (split, b, h) and the merge's slot arithmetic"""
    bad = []
    for gran, dtype in SPLIT_COMBOS[pv]:
        st = C.stack_slots(D, N, False, gran, anchored=True)
        for lens in SPLIT_LENS:
            call = _StackSplit(sa, st, pv, dtype, lens)
            for S in splits:
                _hold_split(call, S, f"{gran}-{lens}", bad)
    assert not bad, bad[:20]


@pytest.mark.parametrize("N,splits", SPLIT_SHAPES, ids=[f"N{n}" for n, _ in SPLIT_SHAPES])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
def test_stacked_split_kv_causal(sa, pv, D, N, splits):
    """sage_attn_fusedq_pv_{f16,f8}_splitkv_causal on the same stacks with q_fold 1 and 2, under the oracle of
    tests/splitkv_causal_util.py per slot: rows without a key exactly 0 / -inf"""
    bad = []
    for gran, dtype in SPLIT_COMBOS[pv]:
        st = C.stack_slots(D, N, False, gran, anchored=True)
        for lens in SPLIT_LENS:
            call = _StackSplit(sa, st, pv, dtype, lens)
            for g in (1, 2):
                for S in splits:
                    o, lse, _, _ = call.run(S, q_fold=g)
                    if torch.isnan(o.float()).any() or torch.isnan(lse).any():
                        bad.append((gran, lens, g, S, "NaN in the result"))
                    for b, n in enumerate(call.lens):
                        for hk in range(st["Hks"]):
                            own, hs = st["grid"][b][hk], C.slot_heads(hk)
                            ro, rl, empty_ok = CU.check(own, pv, n, g, S, o[b:b + 1, hs], lse[b:b + 1, hs], call.qkm(b, hk), o.dtype)
                            _record("splitkv causal", own["family"], pv, D, ro, rl)
                            if not (ro <= 1.0 and rl <= 1.0 and empty_ok):
                                bad.append((gran, lens, g, S, b, hk, ro, rl, empty_ok))
    assert not bad, bad[:20]


_MASK_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}
_KIND = {torch.bool: 1, torch.float16: 2, torch.bfloat16: 3}


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", ["fp16", "bf16"])
def test_stacked_attn_mask(sa, pv, D):
    """sage_attn_qk_int8_pv_f16_masked (per_block with logit_mult_is_one) with the bool and the additive pattern of SMALL_PATTERNS built per slot (slice 2 b + hk
    of a four-slice pattern: no two (b, h) share a mask), 4 and 8 waves"""
    from sageattention_amd import _lib as L
    bad = []
    for gran in C.GRANS:
        st = C.stack_slots(D, 456, False, gran)
        dev = _StackDev(sa, st, pv)
        M, N, fold = st["M"], st["N"], gran == "per_block"
        for name in C.SMALL_PATTERNS:
            pat = C.mask_pattern(name, M, N, _MASK_DTYPE[pv], Bm=4)
            grid = [[C.with_mask(st["grid"][b][hk], pat[2 * b + hk:2 * b + hk + 1]) for hk in range(2)] for b in range(2)]
            mask = torch.cat([torch.cat([c["mask"] for c in row], dim=1) for row in grid], dim=0).contiguous().cuda()
            strides = (ctypes.c_int64 * 4)(*mask.stride())
            for nw in (4, 8):
                o, lse = dev.out()
                with _pinned(nw):
                    L.check(L.lib().sage_attn_qk_int8_pv_f16_masked(
                        _desc(L, dev.q8), _desc(L, dev.k8), _desc(L, dev.v), L.dtype_code(dev.v.dtype), _desc(L, o),
                        L.dtype_code(o.dtype), (dev.qs_folded if fold else dev.qs).data_ptr(), dev.ks.data_ptr(), mask.data_ptr(),
                        _KIND[mask.dtype], strides, lse.data_ptr(), dev.B, dev.Hq, dev.Hk, M, N, D, dev.code, 128,
                        128 if fold else 32, st["sm_scale"], int(fold),
                        L.stream_ptr(o.device)), "masked")
                    torch.cuda.synchronize()
                o, lse = o.cpu(), lse.cpu()
                for b in range(2):
                    for hk in range(2):
                        c, hs = grid[b][hk], C.slot_heads(hk)
                        assert not bool(C.no_key_rows(c).any())
                        ro, rl = C.mask_ratios(c, pv, o[b:b + 1, hs], lse[b:b + 1, hs])
                        _record("mask " + name, c["family"], pv, D, ro, rl)
                        if not (ro <= 1.0 and rl <= 1.0):
                            bad.append((gran, name, nw, b, hk, ro, rl))
    assert not bad, bad[:20]


# ---- b. packed sequences ------------------------------------------------------------------------------------------------------

PAD_ROWS = 70  # poisoned rows in front of and behind every packed window: more than a tile


def _window(t, poison):
    """a packed [rows, H, D] tensor as a window of a poisoned parent -> (device parent, device window)"""
    parent = torch.full((t.shape[0] + 2 * PAD_ROWS,) + tuple(t.shape[1:]), poison, dtype=t.dtype)
    parent[PAD_ROWS:PAD_ROWS + t.shape[0]] = t
    parent = parent.cuda()
    return parent, parent[PAD_ROWS:PAD_ROWS + t.shape[0]]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", ["fp16", "bf16"])
def test_packed_sequences(sa, pv, D):
    """sage_attn_qk_int8_pv_f16_varlen: one call over the sequences of PACK_CUTS -- (150, 456), (64, 65), (1, 1), (129, 320) and
    (33, 0), two KV heads and four query heads cut from different families -- and, causal, of PACK_CUTS_CAUSAL -- M_s < N_s, = and >, top-left -- with 4 and 8
    waves; the scale tensors [S, H, G(max)] with NaN in every unused slot; q8 / k8 / v / o windows of poisoned parents (int8
    127, NaN).  Sequence s is held to its own cut case, the keyless sequence is exactly zero, no element of o is NaN and no
    byte around o changes.  attn_check admits all three granularities for this form (per_block goes in with
    logit_mult_is_one, as the operator calls it), so all three run and there is no refusal to assert."""
    from sageattention_amd import _lib as L
    bad = []
    d3 = lambda t: L.SageTensor(t.data_ptr(), 0, t.stride(1), t.stride(0))
    for gran in C.GRANS:
        for causal in (False, True):
            pk = C.pack_cases(D, gran, causal)
            fold = gran == "per_block"
            _, q8 = _window(pk["q8"], 127)
            _, k8 = _window(pk["k8"], 127)
            _, v = _window(pk["v_f16"] if pv == "fp16" else pk["v_bf16"], NAN)
            qs = (pk["q_scale"] * pk["logit_mult"] if fold else pk["q_scale"]).cuda()
            ks = pk["k_scale"].cuda()
            cu_q, cu_k = pk["cu_q"].cuda(), pk["cu_k"].cuda()
            for nw in (4, 8):
                o_par = torch.full((sum(pk["Ms"]) + 2 * PAD_ROWS, pk["Hq"], D), NAN, dtype=C.OUT_DTYPE[pv], device="cuda")
                o = o_par[PAD_ROWS:PAD_ROWS + sum(pk["Ms"])]
                with _pinned(nw):
                    L.check(L.lib().sage_attn_qk_int8_pv_f16_varlen(
                        d3(q8), d3(k8), d3(v), L.dtype_code(v.dtype), d3(o), L.dtype_code(o.dtype), qs.data_ptr(), ks.data_ptr(),
                        cu_q.data_ptr(), cu_k.data_ptr(), pk["S"], pk["Hq"], pk["Hk"], pk["max_q"], pk["max_k"], D, int(causal),
                        GRAN_CODE[gran], 128, 128 if fold else 32, pk["sm_scale"], int(fold), L.stream_ptr(o.device)), "varlen")
                    torch.cuda.synchronize()
                label = f"{gran}-{'causal' if causal else 'full'}-nw{nw}"
                par = o_par.cpu()
                if not (torch.isnan(par[:PAD_ROWS]).all() and torch.isnan(par[-PAD_ROWS:]).all()):
                    bad.append((label, "rows around o written"))
                oc = par[PAD_ROWS:-PAD_ROWS]
                if torch.isnan(oc.float()).any():
                    bad.append((label, "NaN in o"))
                for s, row in enumerate(pk["cases"]):
                    for hk, own in enumerate(row):
                        os_ = oc[int(pk["cu_q"][s]):int(pk["cu_q"][s + 1]), C.slot_heads(hk)].transpose(0, 1).unsqueeze(0)
                        if own["N"] == 0:
                            if not torch.equal(os_, torch.zeros_like(os_)):
                                bad.append((label, s, hk, "keyless sequence is not zero"))
                            continue
                        ref = C.reference64(own, pv)
                        ro = float(C.ratio_tensors(own, pv, os_, ref["lse2"])[0].max())  # (the entry point has no LSE)
                        _record("packed causal" if causal else "packed", own["family"], pv, D, ro, 0.0)
                        if not ro <= 1.0:
                            bad.append((label, s, hk, own["family"], ro))
    assert not bad, bad[:20]


# ---- c. tile-major K / V ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
def test_tile_major_stack(sa, pv, D):
    """sage_attn_qk_int8_pv_{f16,f8}_kvtiles on the stacked call in the layout of ``tile_major`` ([tiles][B][Hk][64 + 8][D], K
    scales [tiles][B][Hk][8]: every ks_stride non-zero, poison between the tiles and behind the ragged last one), non-causal
    and causal, 4 and 8 waves: within the bound, and o and lse2 bit-identical to the dense entry point on the same stack"""
    from sageattention_amd import _lib as L
    bad = []
    for gran in GRANS2:
        for causal in (False, True):
            st = C.stack_slots(D, 456, causal, gran)
            tm, dev = C.tile_major(st), _StackDev(sa, st, pv)
            k8, ks = tm["k8"].cuda(), tm["k_scale"].cuda()
            if pv == "fp8":
                v8 = tm["v_f8t"].view(torch.uint8).clone()
                v8[..., :64] = fp8_kernel_order(sa, v8[..., :64])
                v, vt = v8.view(torch.float8_e4m3fn).cuda(), tm["v8t"]
            else:
                v, vt = tm["v_f16" if pv == "fp16" else "v_bf16"].cuda(), tm["vt"]
            kd = L.SageTensor(k8.data_ptr(), *tm["kt"][:3])
            vd = L.SageTensor(v.data_ptr(), *vt[:3])
            lay = L.KvLayout(*tm["layout"](pv))
            for nw in (4, 8):
                o, lse = dev.out()
                shape = (dev.B, dev.Hq, dev.Hk, st["M"], st["N"], D, int(causal), dev.code, 128, 32, st["sm_scale"])
                with _pinned(nw):
                    if pv == "fp8":
                        s = L.lib().sage_attn_qk_int8_pv_f8_kvtiles(_desc(L, dev.q8), kd, vd, _desc(L, o), L.dtype_code(o.dtype),
                                                                    dev.qs.data_ptr(), ks.data_ptr(), dev.v_scale.data_ptr(), lay,
                                                                    lse.data_ptr(), *shape, L.stream_ptr(o.device))
                    else:
                        s = L.lib().sage_attn_qk_int8_pv_f16_kvtiles(_desc(L, dev.q8), kd, vd, L.dtype_code(v.dtype), _desc(L, o),
                                                                     L.dtype_code(o.dtype), dev.qs.data_ptr(), ks.data_ptr(), lay,
                                                                     lse.data_ptr(), *shape, L.stream_ptr(o.device))
                    L.check(s, "kvtiles")
                    torch.cuda.synchronize()
                o, lse = o.cpu(), lse.cpu()
                label = f"{gran}-{'causal' if causal else 'full'}-nw{nw}"
                _hold_stack(st, pv, o, lse, "tile-major", label, bad)
                o_d, l_d = dev.run("", causal, nw=nw)
                if not (torch.equal(o.view(torch.int16), o_d.view(torch.int16)) and torch.equal(lse.view(torch.int32), l_d.view(torch.int32))):
                    bad.append((label, "not the bits of the dense entry point"))
    assert not bad, bad[:20]


# ---- d. top-left causal with M != N -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
def test_causal_with_m_not_n(sa, pv, D):
    """(M, N) = (150, 456), (456, 150), (130, 129), causal (top-left: row m keeps the keys n <= m), through the dense int8 entry
    points in both geometries and through the _kvlen twins with full lengths, whose o and lse2 are the dense bits (README)"""
    bad = []
    for gran in C.GRANS:
        for label, c in C.causal_cut_cases(D, gran):
            st = C.stack_of(c)
            dev = _StackDev(sa, st, pv)
            for nw in (4, 8):
                o, lse = dev.run("", True, nw=nw)
                _hold_stack(st, pv, o, lse, "causal M!=N", f"{label}-{gran}-nw{nw}", bad)
                ok, lk = dev.run("kvlen", True, kv_lens=True, nw=nw)
                _hold_stack(st, pv, ok, lk, "causal M!=N kvlen", f"{label}-{gran}-nw{nw}", bad)
                if not (torch.equal(ok.view(torch.int16), o.view(torch.int16)) and torch.equal(lk.view(torch.int32), lse.view(torch.int32))):
                    bad.append((label, gran, nw, "kvlen with full lengths is not the dense bits"))
    assert not bad, bad[:20]


# ---- the checks above notice a misaddressed operand on the device -----------------------------------------------------------

@pytest.mark.parametrize("D", [64, 128])
def test_operands_handed_over_one_slot_off_leave_the_bound(sa, D):
    """No kernel is changed here: the CALLER makes the mistake, with every address still inside the test's own allocations.  The
    stacked dense call with the K-scale rows of the two KV heads exchanged, and the packed call with every cu_seqlens_k entry
    one row up (the rows behind the last sequence are the window's padding): every slot / every sequence with keys must leave
    the bound, as tests/test_constructed_cases.py predicts for head_scales_of_kv_head_0 and cu_off_by_one_row."""
    from sageattention_amd import _lib as L
    pv, gran = "fp16", "per_thread"
    st = C.stack_slots(D, 456, False, gran)
    dev = _StackDev(sa, st, pv)
    dev.ks = dev.ks.flip(1).contiguous()
    o, lse = dev.run("", False, nw=4)
    for b in range(2):
        for hk in range(2):
            hs = C.slot_heads(hk)
            r = max(C.ratios(st["grid"][b][hk], pv, o[b:b + 1, hs], lse[b:b + 1, hs]))
            print(f"K scales of the other KV head, D={D} b{b} hk{hk}: ratio {r:.4g}")
            assert r > 1.0, (b, hk, r)
    pk = C.pack_cases(D, gran, False)
    d3 = lambda t: L.SageTensor(t.data_ptr(), 0, t.stride(1), t.stride(0))
    _, q8 = _window(pk["q8"], 127)
    _, k8 = _window(pk["k8"], 127)
    _, v = _window(pk["v_f16"], 0.0)  # (zeros, not NaN, behind the last key: the ratio printed below stays a number)
    qs, ks, cu_q, cu_k = pk["q_scale"].cuda(), pk["k_scale"].cuda(), pk["cu_q"].cuda(), (pk["cu_k"] + 1).cuda()
    o = torch.full((sum(pk["Ms"]), pk["Hq"], D), NAN, dtype=torch.float16, device="cuda")
    L.check(L.lib().sage_attn_qk_int8_pv_f16_varlen(
        d3(q8), d3(k8), d3(v), L.dtype_code(v.dtype), d3(o), L.dtype_code(o.dtype), qs.data_ptr(), ks.data_ptr(), cu_q.data_ptr(),
        cu_k.data_ptr(), pk["S"], pk["Hq"], pk["Hk"], pk["max_q"], pk["max_k"], D, 0, GRAN_CODE[gran], 128, 32, pk["sm_scale"], 0,
        L.stream_ptr(o.device)), "varlen")
    torch.cuda.synchronize()
    oc = o.cpu()
    for s, row in enumerate(pk["cases"]):
        for hk, own in enumerate(row):
            if own["N"]:
                os_ = oc[int(pk["cu_q"][s]):int(pk["cu_q"][s + 1]), C.slot_heads(hk)].transpose(0, 1).unsqueeze(0)
                r = float(C.ratio_tensors(own, pv, os_, C.reference64(own, pv)["lse2"])[0].max())
                print(f"cu_seqlens_k one row up, D={D} seq{s} hk{hk}: ratio {r:.4g}")
                assert r > 1.0, (s, hk, r)
