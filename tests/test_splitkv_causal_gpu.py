"""Causal split-KV attention on the GPU (``sageattn_splitkv_causal``, ``sage_attn_fusedq_pv_{f16,f8}_splitkv_causal``; the rule:
include/sageattn_hip.h, causal split-KV attention).

1. the constructed operands of tests/constructed_cases.py under the oracle of tests/splitkv_causal_util.py (the bottom-right
   band as a bool mask on the case, the merged bound with the splits a row takes part in): every element of o and of the
   finished LSE at ratio <= 1, rows without keys exactly 0 / -inf;
2. one token (M = 1, g = 1) has the bits of the non-causal operator;
3. len_b = M, one split: the bits of ``sageattn_kvlen(is_causal=True)``, where top-left and bottom-right coincide;
4. a folded call and its unfolded twin, both under the constructed-case bound;
5. the public API: layouts, padded head_dim, strided views, determinism, HIP-graph replay with moved lengths, torch.compile.

o, lse and the caller's workspace are NaN before every C call; K / V rows and K scales beyond len_b are poisoned as in
tests/test_constructed_subsets_gpu.py."""
import pytest
import torch

import constructed_cases as C
import splitkv_causal_util as CU
from constructed_gpu_util import GRAN_CODE, _desc
from test_constructed_subsets_gpu import SPLIT_COMBOS, _k_dev, _v_dev

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
NAN = float("nan")
_RECORD = {}


@pytest.fixture(scope="module")
def sa():
    assert torch.cuda.is_available()
    import sageattention_amd
    import sageattention_amd.ops  # noqa: F401  (registers the ops)
    return sageattention_amd


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    if _RECORD:
        print("\ncausal split-KV on constructed operands: largest |err| / bound over all elements   [o, lse]")
        for (what, fam, pv, D), (ro, rl) in sorted(_RECORD.items()):
            print(f"  {what:8s} {fam:13s} {pv:5s} D={D:<4d} {ro:6.3f} {rl:6.3f}")


def _record(what, fam, pv, D, ro, rl):
    a, b = _RECORD.get((what, fam, pv, D), (0.0, 0.0))
    _RECORD[(what, fam, pv, D)] = (max(a, ro), max(b, rl))


class _CausalCall:
    """sage_attn_fusedq_pv_{f16,f8}_splitkv_causal on an anchored case replicated over batches of the given lengths; the
    query tensor is the caller's (the case's own rows, or a rearrangement of them)"""

    def __init__(self, sa, c, pv, km, lens, q, hq):
        from sageattention_amd import _lib as L
        self.L, self.c, self.pv, self.lens, self.hq = L, c, pv, list(lens), hq
        Bn = self.Bn = len(self.lens)
        self.q = q.expand(Bn, *q.shape[1:]).contiguous().cuda()
        self.km = km.to(q.dtype).expand(Bn, C.HK, c["D"]).contiguous().cuda()
        assert torch.equal(self.km[0].float().cpu(), km[0])
        self.k8, self.ks = _k_dev(c, Bn, self.lens)
        self.v, self.v_scale = _v_dev(sa, c, pv, Bn, self.lens)
        self.kv_lens = torch.tensor(self.lens, dtype=torch.int32, device="cuda")

    def run(self, S, g):
        L, c, Bn = self.L, self.c, self.Bn
        M, N, D = self.q.shape[2], c["N"], c["D"]
        o = torch.full((Bn, self.hq, M, D), NAN, dtype=self.q.dtype, device="cuda")
        lse = torch.full((Bn, self.hq, M), NAN, device="cuda")
        nbytes = L.lib().sage_splitkv_workspace_bytes(Bn, self.hq, M, D, S)
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")  # every fp32 word a NaN
        shape = (Bn, self.hq, C.HK, M, N, D, GRAN_CODE[c["gran"]], 32, c["sm_scale"])
        tail = (self.kv_lens.data_ptr(), S, g, ws.data_ptr(), nbytes, L.stream_ptr(o.device))
        q, k = (_desc(L, self.q), L.dtype_code(self.q.dtype)), _desc(L, self.k8)
        out = (_desc(L, o), L.dtype_code(o.dtype), self.ks.data_ptr(), self.km.data_ptr())
        if self.pv == "fp8":
            st = L.lib().sage_attn_fusedq_pv_f8_splitkv_causal(*q, k, _desc(L, self.v), *out, self.v_scale.data_ptr(), None,
                                                               lse.data_ptr(), *shape, *tail)
        else:
            st = L.lib().sage_attn_fusedq_pv_f16_splitkv_causal(*q, k, _desc(L, self.v), L.dtype_code(self.v.dtype), *out,
                                                                None, lse.data_ptr(), *shape, *tail)
        L.check(st, "splitkv_causal")
        torch.cuda.synchronize()
        return o.cpu(), lse.cpu()


def _hold(c, pv, lens, g, S, o, lse, qkm, what, family, label, bad):
    """every batch of a result against the oracle"""
    if torch.isnan(o.float()).any() or torch.isnan(lse).any():
        bad.append((label, g, S, "NaN in the result"))
    for b, n in enumerate(lens):
        ro, rl, empty_ok = CU.check(c, pv, n, g, S, o[b:b + 1], lse[b:b + 1], qkm, o.dtype)
        print(f"{what} {label} len={n} g={g} S={S}: o {ro:.3f} lse {rl:.3f} rows without keys ok: {empty_ok}")
        _record(what, family, pv, c["D"], ro, rl)
        if not (ro <= 1.0 and rl <= 1.0 and empty_ok):
            bad.append((label, n, g, S, ro, rl, empty_ok))


# ---- 1. constructed operands, every element ---------------------------------------------------------------------------------
CAUSAL_LENGTHS = (None, 257, 100, 0)  # per batch: all keys; off = 107, no multiple of 64; fewer keys than tokens; none
CAUSAL_SPLITS = (1, 2, 3, 5, 8, 16)
CAUSAL_FOLDS = (1, 2, 5)


@pytest.mark.parametrize("N", [512, 456])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("family", C.SPLIT_FAMILIES)
def test_constructed_operands(sa, family, pv, D, N):
    """The split families on the anchored cases, M = 150 (two q-blocks, the second ragged), B = 4 with kv_lens (N, 257, 100, 0),
    every S of (1, 2, 3, 5, 8, 16) with every fold of (1, 2, 5), per_warp and per_thread scales.  At N = 512, S = 8, full
    length, g = 1 (off = 362) wave 0 of q-block 0 ends at key 393 and has no key in split 7 (keys 448..) while waves 2-3 do:
    the clamped wave_tiles."""
    bad = []
    for gran, dtype, km_nonzero in SPLIT_COMBOS[pv]:
        km = C.split_km(D, km_nonzero)
        for label, c in C.split_cases(family, D, N, gran):
            qkm = C.split_qkm(c, km)
            lens = [N if n is None else n for n in CAUSAL_LENGTHS]
            call = _CausalCall(sa, c, pv, km, lens, C.q_real(c, dtype), C.HQ)
            for g in CAUSAL_FOLDS:
                for S in CAUSAL_SPLITS:
                    o, lse = call.run(S, g)
                    _hold(c, pv, lens, g, S, o, lse, qkm, "causal", family, f"{label}-{gran}", bad)
    assert not bad, bad[:20]


# ---- random operands for the bit comparisons ---------------------------------------------------------------------------------
B, HQ, HK = 2, 4, 2


def _make(M, N, D, dtype=torch.float16, seed=0, batches=B):
    g = torch.Generator().manual_seed(1000 * D + 7 * N + M + seed)
    q = torch.randn(batches, HQ, M, D, generator=g)
    k = torch.randn(batches, HK, N, D, generator=g) + 0.5 * torch.randn(batches, HK, 1, D, generator=g)
    v = torch.randn(batches, HK, N, D, generator=g)
    return tuple(t.to(dtype).cuda() for t in (q, k, v))


def _poison(k, v, lens):
    for b, n in enumerate(lens):
        k[b, :, n:] = NAN
        v[b, :, n:] = NAN


def _abi(sa, q, k, v, kv_lens, S, pv, gran, q_fold):
    """the C entry point (causal with ``q_fold``, non-causal with None) on the operands of the operator's own pre-pass, with a
    caller-owned workspace and output pre-filled with NaN"""
    from sageattention_amd import core
    Bq, Hq, M, D = q.shape
    kv = core._prepass(k, v, "HND", gran, True, pv == "fp8", False, kv_lens)
    ws = torch.full((S * Bq * Hq * M * (D + 1) * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full_like(q, NAN)
    o, lse = core._splitkv_attn(q, kv, "HND", (gran, 32), D ** -0.5, True, kv_lens, S, workspace=ws, out=out, q_fold=q_fold)
    torch.cuda.synchronize()
    return o, lse, kv


# ---- 2. one token is the non-causal operator ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_one_token_is_the_non_causal_operator(sa, D, pv):
    """M = 1, g = 1: the token sees every valid key; o and lse equal those of sage_attn_fusedq_pv_*_splitkv bit for bit"""
    lens = [1000, 65, 0]
    q, k, v = _make(1, 1000, D, batches=3)
    _poison(k, v, lens)
    kv_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for S in (2, 5):
        o, lse, _ = _abi(sa, q, k, v, kv_lens, S, pv, "per_thread", 1)
        on, lsen, _ = _abi(sa, q, k, v, kv_lens, S, pv, "per_thread", None)
        assert torch.equal(o, on) and torch.equal(lse, lsen), (D, pv, S)
        assert torch.equal(o[2], torch.zeros_like(o[2])) and bool((lse[2] == NEG_INF).all())
        assert torch.isfinite(o.float()).all() and torch.isfinite(lse[:2]).all()


# ---- 3. the diagonal anchor --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("M", [70, 200])
def test_diagonal_anchor(sa, M, D, pv):
    """kv_lens = M inside a longer poisoned cache, one split, no fold: off = 0, so bottom-right is top-left, and both operators
    run the 4-wave loop over the same tiles -- o has the bits of sageattn_kvlen(is_causal=True).  The two epilogues finish
    the LSE differently (the merge divides and adds in its own order): it is held to the four fp32 roundings of the finish,
    finish_bound with a raw bound of zero."""
    N = M + 190
    q, k, v = _make(M, N, D, seed=5)
    _poison(k, v, [M] * B)
    kv_lens = torch.full((B,), M, dtype=torch.int32, device="cuda")
    o, lse, kv = _abi(sa, q, k, v, kv_lens, 1, pv, "per_thread", 1)
    oref, lref = sa.sageattn_kvlen(q, k, v, kv_lens, is_causal=True, pv=pv, qk_quant_gran="per_thread", return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o, oref), (M, D, pv, int((o != oref).sum()))
    km = kv[2].double().cpu()                                                      # [B,Hk,D]
    qkm = (q.double().cpu() * km.repeat_interleave(HQ // HK, dim=1).unsqueeze(2)).sum(-1) * float(torch.tensor(D ** -0.5))
    lr = lref.double().cpu()
    lse2 = (lr - qkm) * C.K_LOG2E
    l_b = C.finish_bound(torch.zeros_like(lse2), lse2, qkm)
    ratio = float(((lse.double().cpu() - lr).abs() / l_b).max())
    print(f"diagonal anchor M={M} D={D} {pv}: lse ratio {ratio:.3f}")
    assert ratio <= 1.0, (M, D, pv, ratio)


# ---- 4. the fold -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("D", [64, 128])
def test_fold(sa, D, pv):
    """T = 4 tokens, g = 8, N = 1000, kv_lens (1000, 3): the folded call -- 32 rows per KV-side head, q_fold = 8 -- and the
    unfolded one -- the 8 rows of a token as 8 query heads of 4 rows, q_fold = 1 -- rearranged to the folded layout, both
    under the constructed-case bound of the folded band.  (Bit equality is not promised: the waves hold other rows.)  Cases
    with one q scale, so that the fused quantizer returns the same q8 in both layouts: a ramp and a hot last key.  With 3 keys
    for 4 tokens, off = -1: token 0 has no key."""
    T, g, N, lens = 4, 8, 1000, [1000, 3]
    bad = []
    for gran, dtype, km_nonzero in SPLIT_COMBOS[pv]:
        km = C.split_km(D, km_nonzero)
        for label, full in (("ramp6", C.ramp(D, N, False, gran, "6", "ascending", anchor=True)),
                            ("hot999", C.anchor(C.one_hot(D, N, False, gran, N - 1)))):
            c = C.cut_case(full, T * g, N)
            assert c["q_scale_rows"].unique().numel() == 1
            qkm = C.split_qkm(c, km)
            qf = C.q_real(c, dtype)                                              # [1, HQ, T*g, D]: row t*g + i
            qu = qf.view(1, C.HQ, T, g, D).transpose(2, 3).reshape(1, C.HQ * g, T, D)  # head h*g + i, row t
            folded = _CausalCall(sa, c, pv, km, lens, qf, C.HQ)
            unfolded = _CausalCall(sa, c, pv, km, lens, qu, C.HQ * g)
            for S in (1, 4, 16):
                o, lse = folded.run(S, g)
                _hold(c, pv, lens, g, S, o, lse, qkm, "folded", "fold", f"{label}-{gran}", bad)
                ou, lu = unfolded.run(S, 1)
                ou = ou.view(2, C.HQ, g, T, D).transpose(2, 3).reshape(2, C.HQ, T * g, D)
                lu = lu.view(2, C.HQ, g, T).transpose(2, 3).reshape(2, C.HQ, T * g)
                _hold(c, pv, lens, g, S, ou, lu, qkm, "unfolded", "fold", f"{label}-{gran}", bad)
    assert not bad, bad[:20]


# ---- 5. the public API -------------------------------------------------------------------------------------------------------
def _band_ref(q, k, v, lens, g):
    """fp32 softmax under the band, for the plausibility of the public results only (the bounds are tests 1-4's)"""
    Bq, Hq, M, D = q.shape
    out = torch.zeros(Bq, Hq, M, D)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        ok = CU.allowed_keys(n, M, g).cuda()
        kk = k[b, :, :n].float().repeat_interleave(Hq // k.shape[1], dim=0)
        vv = v[b, :, :n].float().repeat_interleave(Hq // k.shape[1], dim=0)
        s = (q[b].float() @ kk.transpose(1, 2)) * D ** -0.5
        p = torch.softmax(s.masked_fill(~ok, NEG_INF), dim=-1)
        out[b] = torch.where(ok.any(-1, keepdim=True), p @ vv, torch.zeros(())).cpu()
    return out


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_nhd_layout_and_plausibility(sa, pv):
    lens = [1000, 40]
    q, k, v = _make(70, 1000, 64)
    _poison(k, v, lens)
    kv_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    o, lse = sa.sageattn_splitkv_causal(q, k, v, kv_lens, 5, 2, pv=pv, return_lse=True)
    qn, kn, vn = (t.transpose(1, 2).contiguous() for t in (q, k, v))
    on, lsen = sa.sageattn_splitkv_causal(qn, kn, vn, kv_lens, 5, 2, tensor_layout="NHD", pv=pv, return_lse=True, is_causal=True)
    torch.cuda.synchronize()
    assert on.shape == qn.shape and torch.equal(on.transpose(1, 2), o) and torch.equal(lsen, lse)
    ref = _band_ref(q, k, v, lens, 2)
    assert torch.isfinite(o.float()).all() and float((o.float().cpu() - ref).abs().max()) < 0.1
    # batch 1: 35 tokens on 40 keys, off = 5 -- every row has keys; the rows of token 0 see 6 of them
    assert torch.isfinite(lse).all()


def test_padded_head_dim(sa):
    """head_dim 72 is padded to 128 with zeros; sm_scale stays that of 72"""
    q, k, v = _make(70, 1000, 72, torch.bfloat16)
    o, lse = sa.sageattn_splitkv_causal(q, k, v, num_splits=3, return_lse=True)
    qp, kp, vp = (torch.nn.functional.pad(t, (0, 56)) for t in (q, k, v))
    op, lsep = sa.sageattn_splitkv_causal(qp, kp, vp, num_splits=3, sm_scale=72 ** -0.5, return_lse=True)
    torch.cuda.synchronize()
    assert o.shape == q.shape and torch.equal(o, op[..., :72]) and torch.equal(lse, lsep)
    assert torch.equal(op[..., 72:], torch.zeros_like(op[..., 72:]))


def test_strided_q_and_o_views(sa):
    """q a view with a row stride of 2 D inside a NaN buffer, o a view inside a buffer of ones: the bits of the contiguous
    call, and nothing outside the view is written"""
    from sageattention_amd import core
    M, N, D, S = 70, 1000, 64, 3
    q, k, v = _make(M, N, D)
    kv_lens = torch.tensor([1000, 30], dtype=torch.int32, device="cuda")
    o_ref, lse_ref = sa.sageattn_splitkv_causal(q, k, v, kv_lens, S, 5, return_lse=True)
    qbuf = torch.full((B, HQ, M, 2 * D), NAN, dtype=q.dtype, device="cuda")
    qbuf[..., :D] = q
    obuf = torch.ones((B, HQ, M + 3, 2 * D), dtype=q.dtype, device="cuda")
    kv = core._prepass(k, v, "HND", "per_thread", True, False, False, kv_lens)
    o, lse = core._splitkv_attn(qbuf[..., :D], kv, "HND", ("per_thread", 32), D ** -0.5, True, kv_lens, S,
                                out=obuf[:, :, :M, D:], q_fold=5)
    torch.cuda.synchronize()
    assert torch.equal(obuf[:, :, :M, D:], o_ref) and torch.equal(lse, lse_ref)
    assert (obuf[:, :, M:] == 1).all() and (obuf[..., :D] == 1).all()
    # batch 1: 14 tokens on 30 keys; nothing missing.  A chunk longer than the cache: the first tokens' rows are 0 / -inf
    short = torch.tensor([1000, 9], dtype=torch.int32, device="cuda")
    o2, l2 = sa.sageattn_splitkv_causal(q, k, v, short, S, 5, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o2[1, :, :25], torch.zeros_like(o2[1, :, :25])) and bool((l2[1, :, :25] == NEG_INF).all())
    assert torch.isfinite(l2[1, :, 25:]).all() and torch.isfinite(o2.float()).all()


def test_two_calls_give_equal_bits(sa):
    q, k, v = _make(200, 1000, 128)
    lens = torch.tensor([1000, 513], dtype=torch.int32, device="cuda")
    a = sa.sageattn_splitkv_causal(q, k, v, lens, 5, 2, pv="fp8", return_lse=True)
    b = sa.sageattn_splitkv_causal(q, k, v, lens, 5, 2, pv="fp8", return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_graph_capture_moves_the_diagonal_at_replay(sa, pv):
    """one captured call, kv_lens overwritten in place, replay: the output of an eager call with the new lengths -- the
    diagonal, the split ranges and the workgroups that run all follow the lengths the tensor holds at replay"""
    first, second = [1000, 100], [64, 0]
    q, k, v = _make(70, 1000, 64, seed=3)
    kv_lens = torch.tensor(first, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sa.sageattn_splitkv_causal(q, k, v, kv_lens, 4, 2, pv=pv, return_lse=True)  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, lg = sa.sageattn_splitkv_causal(q, k, v, kv_lens, 4, 2, pv=pv, return_lse=True)
    for lens in (second, first):
        kv_lens.copy_(torch.tensor(lens, dtype=torch.int32))
        og.fill_(1.0); lg.zero_()
        graph.replay()
        oe, le = sa.sageattn_splitkv_causal(q, k, v, torch.tensor(lens, dtype=torch.int32, device="cuda"), 4, 2, pv=pv,
                                            return_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(og, oe) and torch.equal(lg, le), lens
        assert torch.isfinite(og.float()).all()
    assert not torch.equal(og[0], torch.zeros_like(og[0]))


def test_compile_fullgraph(sa):
    from sageattention_amd.ops import sageattn_splitkv_causal_compilable as f
    q, k, v = _make(70, 1000, 128, seed=4)
    kv_lens = torch.tensor([1000, 0], dtype=torch.int32, device="cuda")
    o, lse = sa.sageattn_splitkv_causal(q, k, v, kv_lens, 3, 2, pv="fp8", return_lse=True)
    oe, le = f(q, k, v, kv_lens, 3, 2, pv="fp8", return_lse=True)
    fn = torch.compile(lambda a, b, c, n: f(a, b, c, n, 3, 2, pv="fp8", return_lse=True), fullgraph=True)
    oc, lc = fn(q, k, v, kv_lens)
    fn0 = torch.compile(lambda a, b, c: f(a, b, c, num_splits=3), fullgraph=True)
    o0 = fn0(q, k, v)
    torch.cuda.synchronize()
    assert torch.equal(oe, o) and torch.equal(le, lse) and torch.equal(oc, o) and torch.equal(lc, lse)
    assert torch.equal(o0, sa.sageattn_splitkv_causal(q, k, v, num_splits=3))
    assert torch.equal(o[1], torch.zeros_like(o[1])) and torch.isfinite(o.float()).all()
