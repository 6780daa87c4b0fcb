"""The kernels that compute on a SUBSET of the keys -- block-sparse attention under real maps, per-batch key lengths, split-KV
-- on the constructed int8 operands and scales of tests/constructed_cases.py, against the fp64 softmax of exactly the keys
the call attends and the derived per-element bounds (``bound`` on ``subcase``; ``merged_bound`` for the split-KV merge;
tests/test_constructed_cases.py proves on the CPU that they are sound and have teeth).  A constructed case restricted to
some of its 64-key tiles is again a constructed case, so one mechanism serves all three.  Every entry point is called through
the C ABI; every element of o and of the LSE is held to ratio <= 1: no percentile, no skipped case.

Why constructed operands: a mistake in the K-scale offset of a split, in the tile a list entry names or in the ragged tail at
len_b shows only when neighbouring tiles carry DIFFERENT scales (scale_ladder), and the split-KV merge leaves its
near-uniform weights only when the attention itself produces LSEs that differ (the step-40 ramps: gaps between the splits'
LSEs below 1, 1..24, 24..126, 126..149 -- fp32 weights subnormal -- and above 150, the dominant split first, in the middle and
last; ``offset``: LSEs of 2^10 and more with gaps below 1).  tests/test_constructed_cases.py asserts those regimes from the fp64
reference alone.

Poison: K rows beyond a batch's length hold int8 127 and their K scales NaN, fp16 / bf16 V rows NaN.  The e4m3 V^T holds 0x7F
(NaN) from column 64 * ceil(len_b / 64) on and ZEROS in [len_b, 64 * ceil(len_b / 64)): that is the operand the contract
names (sage_kv_prepare_fp8_kvlen writes those zeros; the kernel's descriptor covers the whole last tile)."""
import pytest
import torch

import constructed_cases as C
from constructed_gpu_util import GRAN_CODE, _desc, _pinned

pytestmark = pytest.mark.gpu

_RECORD = {}
NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def sa():
    assert torch.cuda.is_available()
    import sageattention_amd
    return sageattention_amd


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    if _RECORD:
        print("\nconstructed subsets: largest |err| / bound over all elements   [o, lse]")
        for (what, fam, pv, D), (ro, rl) in sorted(_RECORD.items()):
            print(f"  {what:14s} {fam:13s} {pv:5s} D={D:<4d} {ro:6.3f} {rl:6.3f}")


def _record(what, fam, pv, D, ro, rl):
    a, b = _RECORD.get((what, fam, pv, D), (0.0, 0.0))
    _RECORD[(what, fam, pv, D)] = (max(a, ro), max(b, rl))


def _v_dev(sa, c, pv, Bn, lens):
    """V of the case replicated over Bn batches, poisoned beyond each batch's length -> (device tensor, v_scale or None)"""
    N = c["N"]
    if pv != "fp8":
        v = C.v_of(c, pv).expand(Bn, C.HK, N, c["D"]).clone()
        for b, n in enumerate(lens):
            v[b, :, n:] = float("nan")
        return v.cuda(), None
    v8 = c["v_f8t"].view(torch.uint8).expand(Bn, C.HK, c["D"], -1).clone()  # tokens in natural order
    for b, n in enumerate(lens):
        v8[b, :, :, n:] = 0
        v8[b, :, :, (n + 63) // 64 * 64:] = 0x7F
    perm = sa.quant.fp8_token_order()
    idx = (torch.arange(v8.shape[-1] // 64).view(-1, 1) * 64 + perm.view(1, -1)).reshape(-1)  # position -> token
    return v8[..., idx].contiguous().view(torch.float8_e4m3fn).cuda(), c["v_scale"].expand(Bn, C.HK, -1).contiguous().cuda()


def _k_dev(c, Bn, lens):
    """k8 and the compact k_scale replicated, int8 127 in the rows beyond each length, NaN in the scales of the tiles wholly
    beyond it"""
    k8 = c["k8"].expand(Bn, C.HK, c["N"], c["D"]).clone()
    ks = c["k_scale"].expand(Bn, C.HK, -1).clone()
    per = ks.shape[-1] // ((c["N"] + 63) // 64)
    for b, n in enumerate(lens):
        k8[b, :, n:] = 127
        ks[b, :, (n + 63) // 64 * per:] = float("nan")
    return k8.cuda(), ks.cuda()


class _Int8Call:
    """the int8-Q entry points (block-sparse, kvlen, block-sparse + kvlen) on one case replicated over Bn batches"""

    def __init__(self, sa, c, pv, lens):
        from sageattention_amd import _lib as L
        self.L, self.c, self.pv, self.Bn = L, c, pv, len(lens)
        Bn = self.Bn
        self.q8 = c["q8"].expand(Bn, C.HQ, c["M"], c["D"]).contiguous().cuda()
        self.qs = c["q_scale"].expand(Bn, C.HQ, -1).contiguous().cuda()
        self.k8, self.ks = _k_dev(c, Bn, lens)
        self.v, self.v_scale = _v_dev(sa, c, pv, Bn, lens)
        self.kv_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")

    def run(self, name, causal=False, lists=None, kv_lens=False):
        L, c = self.L, self.c
        M, N, D = c["M"], c["N"], c["D"]
        o = torch.full((self.Bn, C.HQ, M, D), float("nan"), dtype=C.OUT_DTYPE[self.pv], device="cuda")
        lse = torch.full((self.Bn, C.HQ, M), float("nan"), device="cuda")
        head = (_desc(L, self.q8), _desc(L, self.k8), _desc(L, self.v))
        mid = (_desc(L, o), L.dtype_code(o.dtype), self.qs.data_ptr(), self.ks.data_ptr())
        warpq = 128 if c["gran"] == "per_block" else 32
        tail = (None, lse.data_ptr(), self.Bn, C.HQ, C.HK, M, N, D, int(causal), GRAN_CODE[c["gran"]], 128, warpq,
                c["sm_scale"], 0)
        if lists is not None:
            tail += (lists.data_ptr(), lists.numel() * 4)
            if kv_lens:
                tail += (None, None)  # pv_thresh, skipped: the kernel without the P.V skip
        if kv_lens:
            tail += (self.kv_lens.data_ptr(),)
        tail += (L.stream_ptr(o.device),)
        if self.pv == "fp8":
            st = getattr(L.lib(), f"sage_attn_qk_int8_pv_f8_{name}")(*head, *mid, self.v_scale.data_ptr(), *tail)
        else:
            st = getattr(L.lib(), f"sage_attn_qk_int8_pv_f16_{name}")(*head, L.dtype_code(self.v.dtype), *mid, *tail)
        L.check(st, name)
        torch.cuda.synchronize()
        return o.cpu(), lse.cpu()


def _rows(qb, M):
    return slice(128 * qb, min(128 * qb + 128, M))


def _check_map(c, pv, o, lse, b, tiles_of, length, what, family, label, bad):
    """batch b of a block-sparse result: every (head, q-block) against the subcase of its tile list clipped to ``length``"""
    for h in range(C.HQ):
        for qb in range(2):
            tiles = [t for t in tiles_of[h][qb] if 64 * t < (c["N"] if length is None else length)]
            rs = _rows(qb, c["M"])
            if not tiles:  # no tile below the length: the convention of empty q-blocks
                if not (torch.equal(o[b, h, rs], torch.zeros_like(o[b, h, rs])) and bool((lse[b, h, rs] == NEG_INF).all())):
                    bad.append((label, what, b, h, qb, "empty q-block is not 0 / -inf"))
                continue
            d = C.cached_subcase(c, tiles, length)
            ro, rl = C.ratio_tensors(d, pv, o[b:b + 1], lse[b:b + 1])
            ro, rl = float(ro[0, h, rs].max()), float(rl[0, h, rs].max())
            _record(what, family, pv, c["D"], ro, rl)
            if not (ro <= 1.0 and rl <= 1.0):
                bad.append((label, what, b, h, qb, tiles, ro, rl))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("family", C.SUBSET_FAMILIES)
def test_block_sparse_under_real_maps(sa, family, pv, D):
    """sage_attn_qk_int8_pv_{f16,f8}_blocksparse at N = 456 under the maps of constructed_cases.SUBSET_MAPS: every other tile,
    only the ragged tile, first + last, one middle tile, and a map that differs between the q-blocks and between the heads.
    one_hot: each map lists the hot key's tile for some of the cases and not for the others (asserted)."""
    bad, listed = [], set()
    for label, c in C.subset_cases(family, D, pv, C.GRANS):
        call = _Int8Call(sa, c, pv, [c["N"]])
        for name, tiles_of in C.SUBSET_MAPS.items():
            lists = sa.block_sparse_plan(C.map_tensor(name).cuda(), c["M"], c["N"], B=1, Hq=C.HQ).lists
            o, lse = call.run("blocksparse", lists=lists)
            _check_map(c, pv, o, lse, 0, tiles_of, None, "sparse", family, f"{label}-{name}", bad)
            if family == "one_hot":
                listed.add((name, c["hot"] // 64 in tiles_of[0][0]))
    if family == "one_hot":
        assert all((name, True) in listed and (name, False) in listed for name in C.SUBSET_MAPS), listed
    assert not bad, bad[:20]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("family", C.SUBSET_FAMILIES)
def test_dense_with_kv_lens(sa, family, pv, D):
    """sage_attn_qk_int8_pv_{f16,f8}_kvlen: the case replicated over B = 4 with lengths (N, 257, 64, 1), causal and not, both
    wave geometries, poison beyond every length; batch b against subcase(c, length=len_b)"""
    bad = []
    lens = list(C.KVLEN_LENGTHS)
    for causal in (False, True):
        for label, c in C.subset_cases(family, D, pv, ("per_warp", "per_thread"), causal):
            call = _Int8Call(sa, c, pv, lens)
            for nw in (4, 8):
                with _pinned(nw):
                    o, lse = call.run("kvlen", causal=causal, kv_lens=True)
                for b, n in enumerate(lens):
                    d = C.cached_subcase(c, None, n)
                    ro, rl = C.ratios(d, pv, o[b:b + 1], lse[b:b + 1])
                    _record("kvlen", family, pv, D, ro, rl)
                    if not (ro <= 1.0 and rl <= 1.0):
                        bad.append((label, nw, n, ro, rl))
    assert not bad, bad[:20]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("family", C.SUBSET_FAMILIES)
def test_block_sparse_with_kv_lens(sa, family, pv, D):
    """sage_attn_qk_int8_pv_{f16,f8}_blocksparse_kvlen under the partial maps "alternate" and "mixed" with the lengths
    (N, 257, 64, 1): each list is clipped to the batch's tiles, and where it lists the tile that holds key len_b - 1 ("mixed":
    tile 4 at 257, tile 0 at 64 and 1) that tile is ragged at len_b; a q-block that lists (1, 3, 5, 7) has no tile below the
    lengths 64 and 1 and must hold 0 / -inf"""
    bad = []
    lens = list(C.KVLEN_LENGTHS)
    for label, c in C.subset_cases(family, D, pv, ("per_warp", "per_thread")):
        call = _Int8Call(sa, c, pv, lens)
        for name in ("alternate", "mixed"):
            bm = C.map_tensor(name).expand(len(lens), -1, -1, -1).contiguous().cuda()
            lists = sa.block_sparse_plan(bm, c["M"], c["N"], B=len(lens), Hq=C.HQ).lists
            o, lse = call.run("blocksparse_kvlen", lists=lists, kv_lens=True)
            for b, n in enumerate(lens):
                _check_map(c, pv, o, lse, b, C.SUBSET_MAPS[name], n, "sparse+kvlen", family, f"{label}-{name}-len{n}", bad)
    assert not bad, bad[:20]


# ---- split-KV ------------------------------------------------------------------------------------------------------------

# (granularity, Q / output dtype, non-zero km) per PV type: fp16 / bf16 V go with Q of their own type, as in the operator
SPLIT_COMBOS = {
    "fp16": (("per_warp", torch.float16, False), ("per_thread", torch.float16, True)),
    "bf16": (("per_warp", torch.bfloat16, True), ("per_thread", torch.bfloat16, False)),
    "fp8": (("per_warp", torch.float16, True), ("per_thread", torch.bfloat16, False)),
}


class _SplitCall:
    """sage_attn_fusedq_pv_{f16,f8}_splitkv on an anchored case replicated over the batches of SPLIT_LENGTHS"""

    def __init__(self, sa, c, pv, dtype, km, rows):
        from sageattention_amd import _lib as L
        self.L, self.c, self.pv, self.rows = L, c, pv, rows
        self.lens = [c["N"] if n is None else n for n in C.SPLIT_LENGTHS]
        Bn = self.Bn = len(self.lens)
        self.q = C.q_real(c, dtype)[:, :, :rows].expand(Bn, C.HQ, rows, c["D"]).contiguous().cuda()
        self.km = km.to(dtype).expand(Bn, C.HK, c["D"]).contiguous().cuda()
        assert torch.equal(self.km[0].float().cpu(), km[0])
        self.k8, self.ks = _k_dev(c, Bn, self.lens)
        self.v, self.v_scale = _v_dev(sa, c, pv, Bn, self.lens)
        self.kv_lens = torch.tensor(self.lens, dtype=torch.int32, device="cuda")

    def run(self, S):
        """-> (o, lse, o_parts fp32 [S,B,Hq,rows,D], lse2_parts fp32 [S,B,Hq,rows]) on the CPU; the workspace is the caller's,
        every fp32 word of it a NaN beforehand"""
        L, c, Bn, M = self.L, self.c, self.Bn, self.rows
        N, D = c["N"], c["D"]
        o = torch.full((Bn, C.HQ, M, D), float("nan"), dtype=self.q.dtype, device="cuda")
        lse = torch.full((Bn, C.HQ, M), float("nan"), device="cuda")
        nbytes = L.lib().sage_splitkv_workspace_bytes(Bn, C.HQ, M, D, S)
        assert nbytes == S * Bn * C.HQ * M * (D + 1) * 4
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
        shape = (Bn, C.HQ, C.HK, M, N, D, GRAN_CODE[c["gran"]], 32, c["sm_scale"])
        tail = (self.kv_lens.data_ptr(), S, ws.data_ptr(), nbytes, L.stream_ptr(o.device))
        q, k = (_desc(L, self.q), L.dtype_code(self.q.dtype)), _desc(L, self.k8)
        out = (_desc(L, o), L.dtype_code(o.dtype), self.ks.data_ptr(), self.km.data_ptr())
        if self.pv == "fp8":
            st = L.lib().sage_attn_fusedq_pv_f8_splitkv(*q, k, _desc(L, self.v), *out, self.v_scale.data_ptr(), None,
                                                        lse.data_ptr(), *shape, *tail)
        else:
            st = L.lib().sage_attn_fusedq_pv_f16_splitkv(*q, k, _desc(L, self.v), L.dtype_code(self.v.dtype), *out, None,
                                                         lse.data_ptr(), *shape, *tail)
        L.check(st, "splitkv")
        torch.cuda.synchronize()
        f = ws.view(torch.float32).cpu()
        n_o = S * Bn * C.HQ * M * D
        return o.cpu(), lse.cpu(), f[:n_o].view(S, Bn, C.HQ, M, D), f[n_o:].view(S, Bn, C.HQ, M)


def _check_split(call, S, qkm, family, label, bad):
    c, pv, rows = call.c, call.pv, call.rows
    o, lse, o_parts, l2_parts = call.run(S)
    tag = "splitkv" if rows > 1 else "splitkv-M1"
    if torch.isnan(o.float()).any() or torch.isnan(lse).any():
        bad.append((label, S, "NaN in the result"))
    cut = lambda t: t[:, :, :rows]
    for b, n in enumerate(call.lens):
        if n == 0:  # a batch without keys: exactly 0 and -inf, every slot of the workspace untouched
            if not (torch.equal(o[b], torch.zeros_like(o[b])) and bool((lse[b] == NEG_INF).all())):
                bad.append((label, S, b, "batch without keys is not 0 / -inf"))
            if not (torch.isnan(o_parts[:, b]).all() and torch.isnan(l2_parts[:, b]).all()):
                bad.append((label, S, b, "workspace of a batch without keys written"))
            continue
        cn = c if n == c["N"] else C.cached_subcase(c, None, n)
        subs = C.split_subcases(cn, S)
        for s in range(S):
            if s >= len(subs):
                if not (torch.isnan(o_parts[s, b]).all() and torch.isnan(l2_parts[s, b]).all()):
                    bad.append((label, S, b, s, "slot of an empty split written"))
                continue
            ref = C.reference64(subs[s], pv)
            o_b, l_b = C.bound(subs[s], pv, out_ulps=0)
            po, pl = o_parts[s, b:b + 1].double(), l2_parts[s, b:b + 1].double()
            ok = bool(torch.isfinite(po).all() and torch.isfinite(pl).all())
            ro = float(((po - cut(ref["o"])).abs() / cut(o_b)).max()) if ok else float("inf")
            rl = float(((pl - cut(ref["lse2"])).abs() / cut(l_b)).max()) if ok else float("inf")
            _record(tag + " part", family, pv, c["D"], ro, rl)
            if not (ro <= 1.0 and rl <= 1.0):
                bad.append((label, S, b, s, "partial", ro, rl))
        ref = C.reference64(cn, pv)
        o_b, l2_b = C.merged_bound(cn, pv, S, o.dtype)
        l_b = C.finish_bound(l2_b, ref["lse2"], qkm)
        go, gl = o[b:b + 1].double(), lse[b:b + 1].double()
        ok = bool(torch.isfinite(go).all() and torch.isfinite(gl).all())
        ro = float(((go - cut(ref["o"])).abs() / cut(o_b)).max()) if ok else float("inf")
        rl = float(((gl - cut(C.finish_lse64(ref["lse2"], qkm))).abs() / cut(l_b)).max()) if ok else float("inf")
        _record(tag, family, pv, c["D"], ro, rl)
        if not (ro <= 1.0 and rl <= 1.0):
            bad.append((label, S, b, "merged", ro, rl))


@pytest.mark.parametrize("N,splits", C.SPLIT_CONFIGS, ids=[f"N{n}" for n, _ in C.SPLIT_CONFIGS])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("family", C.SPLIT_FAMILIES)
def test_split_kv_partials_and_merge(sa, family, pv, D, N, splits):
    """sage_attn_fusedq_pv_{f16,f8}_splitkv on the ANCHORED cases (the fused quantizer returns the chosen q8 and 2^e exactly),
    B = 3 with kv_lens (N, 257, 0) and poison beyond them, a caller-owned workspace of NaN bytes, km zeros or multiples of 1/8.
    N = 512: S in 2, 3, 4, 5, 8, 9, 16 -- 4, 3, 2, 2, 1, 1, 1 tiles per split, 2..8 non-empty splits, every MAXC of the merge;
    N = 456: S in 2, 3, 7 for the ragged last split.  Checked: every non-empty partial of the workspace under ``bound`` of its
    subcase (fp32: no output ulps), the slots of empty splits still NaN, the merged o and the finished LSE under
    ``merged_bound`` / ``finish_bound``, the batch without keys exactly 0 / -inf, no NaN.  Then the first r = 4 row alone
    (M = 1), the shape the operator was written for."""
    bad = []
    for gran, dtype, km_nonzero in SPLIT_COMBOS[pv]:
        km = C.split_km(D, km_nonzero)
        for label, c in C.split_cases(family, D, N, gran):
            qkm = C.split_qkm(c, km)
            assert bool((qkm != 0).any()) == km_nonzero
            runs = [C.M_FULL] + ([1] if gran == "per_warp" else [])
            for rows in runs:
                call = _SplitCall(sa, c, pv, dtype, km, rows)
                for S in splits:
                    _check_split(call, S, qkm, family, f"{label}-{gran}-M{rows}", bad)
    assert not bad, bad[:20]
