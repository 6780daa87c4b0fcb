"""Split-KV attention on the GPU (``sageattn_splitkv``; the rule: include/sageattn_hip.h, split-KV attention).

The oracle of a split's partial result is the existing public operator ``sageattn_block_sparse`` called with a map that is on
in exactly the split's tile columns for every q-block (tests/splitkv_util.py): the rule says the fp32 partial in the workspace,
rounded to the output dtype, has that operator's bits -- ``torch.equal``, no tolerance.  The final result is checked against the
fp64 merge of those oracle partials with the derived bound of tests/seqpar_ref.py.  B = 2, Hq = 4 on Hk = 2 (GQA)."""
import pytest
import torch

import seqpar_ref as R
import splitkv_util as SU

pytestmark = pytest.mark.gpu

B, HQ, HK = 2, 4, 2
NEG_INF = float("-inf")
NAN = float("nan")


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    import sageattention_amd.ops  # noqa: F401  (registers the ops)
    return sageattention_amd


def _make(M, N, D, dtype=torch.float16, seed=0):
    """seeded q, k, v (HND) on the GPU; k carries a per-channel offset, so that the smoothing mean matters"""
    g = torch.Generator().manual_seed(1000 * D + 7 * N + M + seed)
    q = torch.randn(B, HQ, M, D, generator=g)
    k = torch.randn(B, HK, N, D, generator=g) + 0.5 * torch.randn(B, HK, 1, D, generator=g)
    v = torch.randn(B, HK, N, D, generator=g)
    return tuple(t.to(dtype).cuda() for t in (q, k, v))


def _poison(k, v, lens):
    """NaN into the K and V rows >= len_b (HND)"""
    for b, n in enumerate(lens):
        k[b, :, n:] = NAN
        v[b, :, n:] = NAN


def _run_abi(sa, q, k, v, kv_lens, S, pv, gran):
    """the C entry point on the operands of the operator's own pre-pass, with a caller-owned workspace pre-filled with NaN bytes
    -> (o, lse, o_parts fp32 [S,B,Hq,M,D], lse2_parts fp32 [S,B,Hq,M])"""
    from sageattention_amd import core
    qp, kp, vp, d_og = core._pad_head_dim(q, k, v)
    assert d_og == q.size(-1) == qp.size(-1)
    Bq, Hq, M, D = qp.shape
    kv = core._prepass(kp, vp, "HND", gran, True, pv == "fp8", False, kv_lens)
    nbytes = S * Bq * Hq * M * (D + 1) * 4
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")  # every fp32 word a NaN
    o, lse = core._splitkv_attn(qp, kv, "HND", (gran, 32), D ** -0.5, True, kv_lens, S, workspace=ws)
    torch.cuda.synchronize()
    f = ws.view(torch.float32)
    n_o = S * Bq * Hq * M * D
    return o, lse, f[:n_o].view(S, Bq, Hq, M, D), f[n_o:].view(S, Bq, Hq, M)


def _oracle_parts(sa, q, k, v, kv_lens, lens, S, pv, gran):
    """``sageattn_block_sparse`` under the column-range map of every split -> ([o_s], [lse_s]); a batch in which split s is
    empty has o_s = 0 and lse_s = -inf there (the operator's convention for q-blocks without a tile)"""
    M, N = q.size(2), k.size(2)
    os_, ls = [], []
    for s in range(S):
        bm = SU.range_map(lens, N, M, HQ, S, s).cuda()
        kw = {} if kv_lens is None else dict(kv_lens=kv_lens)
        o_s, l_s = sa.sageattn_block_sparse(q, k, v, bm, pv=pv, qk_quant_gran=gran, return_lse=True, **kw)
        os_.append(o_s)
        ls.append(l_s)
    torch.cuda.synchronize()
    return os_, ls


def _check_case(sa, M, N, D, S, pv, gran, dtype, raw_lens=None, seed=0):
    """(a) every non-empty partial bit for bit, the slots of empty splits untouched; (b) the final result within the derived
    bound of the fp64 merge of the oracle partials, -inf and 0 exactly where a batch has no keys, no NaN anywhere"""
    q, k, v = _make(M, N, D, dtype, seed)
    lens = [N] * B if raw_lens is None else [SU.clamp_len(x, N) for x in raw_lens]
    kv_lens = None if raw_lens is None else torch.tensor(raw_lens, dtype=torch.int32, device="cuda")
    if raw_lens is not None:
        _poison(k, v, lens)
    tag = (M, N, D, S, pv, gran, dtype, raw_lens)
    o, lse, o_parts, l2_parts = _run_abi(sa, q, k, v, kv_lens, S, pv, gran)
    os_, ls = _oracle_parts(sa, q, k, v, kv_lens, lens, S, pv, gran)
    # (a)
    for b, n in enumerate(lens):
        cnt = SU.nonempty_splits(n, S)
        for s in range(S):
            if s < cnt:
                assert torch.isfinite(o_parts[s, b]).all() and torch.isfinite(l2_parts[s, b]).all(), (tag, b, s)
                got = o_parts[s, b].to(dtype)
                assert torch.equal(got, os_[s][b]), (tag, b, s, int((got != os_[s][b]).sum()))
                assert torch.isfinite(ls[s][b]).all(), (tag, b, s)
            else:
                assert torch.isnan(o_parts[s, b]).all() and torch.isnan(l2_parts[s, b]).all(), (tag, b, s, "slot of an empty split written")
                assert torch.equal(ls[s][b], torch.full_like(ls[s][b], NEG_INF)), (tag, b, s)
    # (b)
    ref, o_extra = SU.merged_reference(os_, ls, dtype, o.reshape(-1, D))
    R.check_merge(o.cpu().reshape(-1, D), lse.cpu().reshape(-1), ref, dtype, o_extra=o_extra)
    for b, n in enumerate(lens):
        if n == 0:
            assert torch.equal(o[b], torch.zeros_like(o[b])) and torch.equal(lse[b], torch.full_like(lse[b], NEG_INF)), (tag, b)
    assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any(), tag


CONFIGS = [(D, pv, gran, dtype) for D in (64, 128) for pv in ("fp16", "fp8") for gran in ("per_thread", "per_warp")
           for dtype in (torch.float16, torch.bfloat16)]
IDS = [f"d{d}-{pv}-{g}-{'bf16' if dt == torch.bfloat16 else 'fp16'}" for d, pv, g, dt in CONFIGS]
# N = 1000: 16 tiles with a ragged tail (tps 8, 6, 4, 1: S = 3 ends with a short split, S = 5 leaves the fifth empty,
# S = 16 gives every tile its own workgroup; S = 4 and 8: tps 4 and 2, every slot of MAXC = 4 / 8 in use; S = 9: tps 2, so
# MAXC = 16 with 8 non-empty slots); N = 130 with S = 8: more splits than tiles
SPLITS = [(1000, 2), (1000, 3), (1000, 4), (1000, 5), (1000, 8), (1000, 9), (1000, 16), (130, 8)]


@pytest.mark.parametrize("M", [1, 70, 200])
@pytest.mark.parametrize("D,pv,gran,dtype", CONFIGS, ids=IDS)
def test_partials_and_merge(sa, D, pv, gran, dtype, M):
    for N, S in SPLITS:
        _check_case(sa, M, N, D, S, pv, gran, dtype)


@pytest.mark.parametrize("raw_lens", [[1000, 0], [65, 513], [64, 1], [-5, 1100]], ids=["1000-0", "65-513", "64-1", "clamped"])
@pytest.mark.parametrize("D,pv,gran,dtype", CONFIGS, ids=IDS)
def test_kv_lens(sa, D, pv, gran, dtype, raw_lens):
    """per-batch lengths with NaN in every K and V row beyond them: a batch without keys, a length one past a tile edge, a whole
    tile, a single key; values outside [0, N] clamp"""
    for M, S in ((70, 2), (200, 3), (1, 5), (70, 16)):
        _check_case(sa, M, 1000, D, S, pv, gran, dtype, raw_lens=raw_lens)


# ---- (c) layouts and views -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_nhd_layout(sa, pv):
    q, k, v = _make(70, 1000, 64)
    lens = torch.tensor([1000, 513], dtype=torch.int32, device="cuda")
    o, lse = sa.sageattn_splitkv(q, k, v, lens, 5, pv=pv, return_lse=True)
    qn, kn, vn = (t.transpose(1, 2).contiguous() for t in (q, k, v))
    on, lsen = sa.sageattn_splitkv(qn, kn, vn, lens, 5, tensor_layout="NHD", pv=pv, return_lse=True)
    torch.cuda.synchronize()
    assert on.shape == qn.shape and torch.equal(on.transpose(1, 2), o) and torch.equal(lsen, lse)


def test_padded_head_dim(sa):
    """head_dim 72 is padded to 128 with zeros; sm_scale stays that of 72"""
    q, k, v = _make(70, 1000, 72, torch.bfloat16)
    o, lse = sa.sageattn_splitkv(q, k, v, num_splits=3, return_lse=True)
    qp, kp, vp = (torch.nn.functional.pad(t, (0, 56)) for t in (q, k, v))
    op, lsep = sa.sageattn_splitkv(qp, kp, vp, num_splits=3, sm_scale=72 ** -0.5, return_lse=True)
    torch.cuda.synchronize()
    assert o.shape == q.shape and torch.equal(o, op[..., :72]) and torch.equal(lse, lsep)
    assert torch.equal(op[..., 72:], torch.zeros_like(op[..., 72:]))


def test_strided_q_and_o_views(sa):
    """q a view with a row stride of 2 D inside a NaN buffer, o a view with a row stride of 2 D and a head stride with a gap
    inside a buffer of ones: the bits of the contiguous call, and nothing outside the view is written"""
    from sageattention_amd import core
    M, N, D, S = 70, 1000, 64, 3
    q, k, v = _make(M, N, D)
    o_ref, lse_ref = sa.sageattn_splitkv(q, k, v, num_splits=S, return_lse=True)
    qbuf = torch.full((B, HQ, M, 2 * D), NAN, dtype=q.dtype, device="cuda")
    qbuf[..., :D] = q
    obuf = torch.ones((B, HQ, M + 3, 2 * D), dtype=q.dtype, device="cuda")
    kv = core._prepass(k, v, "HND", "per_thread", True, False, False, None)
    o, lse = core._splitkv_attn(qbuf[..., :D], kv, "HND", ("per_thread", 32), D ** -0.5, True, None, S, out=obuf[:, :, :M, D:])
    torch.cuda.synchronize()
    assert torch.equal(obuf[:, :, :M, D:], o_ref) and torch.equal(lse, lse_ref)
    assert (obuf[:, :, M:] == 1).all() and (obuf[..., :D] == 1).all()


# ---- (d) a resolved count of 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_one_split_is_the_operator_it_names(sa, pv):
    from sageattention_amd import core
    q, k, v = _make(200, 130, 64)
    assert core.splitkv_num_splits(B, HQ, 200, 130) == 1
    dense = sa.sageattn_qk_int8_pv_fp8_cuda if pv == "fp8" else sa.sageattn_qk_int8_pv_fp16_cuda
    od, ld = dense(q, k, v, return_lse=True)
    for ns in (None, 1):
        o, lse = sa.sageattn_splitkv(q, k, v, num_splits=ns, pv=pv, return_lse=True)
        assert torch.equal(o, od) and torch.equal(lse, ld)
    lens = torch.tensor([77, 0], dtype=torch.int32, device="cuda")
    ok, lk = sa.sageattn_kvlen(q, k, v, lens, pv=pv, return_lse=True)
    o, lse = sa.sageattn_splitkv(q, k, v, lens, pv=pv, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o, ok) and torch.equal(lse, lk)
    assert torch.equal(sa.sageattn_splitkv(q, k, v, lens, 1, pv=pv), ok)


# ---- (e) determinism -------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits(sa):
    q, k, v = _make(200, 1000, 128)
    lens = torch.tensor([1000, 513], dtype=torch.int32, device="cuda")
    a = sa.sageattn_splitkv(q, k, v, lens, 5, pv="fp8", return_lse=True)
    b = sa.sageattn_splitkv(q, k, v, lens, 5, pv="fp8", return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- (f) HIP-graph capture ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_graph_capture_reads_the_lengths_at_replay(sa, pv):
    """one captured call, kv_lens overwritten in place, replay: the output of an eager call with the new lengths"""
    first, second = [1000, 100], [64, 0]
    q, k, v = _make(70, 1000, 64, seed=3)
    kv_lens = torch.tensor(first, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sa.sageattn_splitkv(q, k, v, kv_lens, 4, pv=pv, return_lse=True)  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, lg = sa.sageattn_splitkv(q, k, v, kv_lens, 4, pv=pv, return_lse=True)
    for lens in (second, first):
        kv_lens.copy_(torch.tensor(lens, dtype=torch.int32))
        og.fill_(1.0); lg.zero_()
        graph.replay()
        oe, le = sa.sageattn_splitkv(q, k, v, torch.tensor(lens, dtype=torch.int32, device="cuda"), 4, pv=pv, return_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(og, oe) and torch.equal(lg, le), lens
        assert torch.isfinite(og.float()).all()


# ---- (g) torch.compile -------------------------------------------------------------------------------------------------------
def test_compile_fullgraph(sa):
    from sageattention_amd.ops import sageattn_splitkv_compilable
    q, k, v = _make(70, 1000, 128, seed=4)
    kv_lens = torch.tensor([1000, 0], dtype=torch.int32, device="cuda")
    o, lse = sa.sageattn_splitkv(q, k, v, kv_lens, 3, pv="fp8", return_lse=True)
    oe, le = sageattn_splitkv_compilable(q, k, v, kv_lens, 3, pv="fp8", return_lse=True)
    fn = torch.compile(lambda a, b, c, n: sageattn_splitkv_compilable(a, b, c, n, 3, pv="fp8", return_lse=True), fullgraph=True)
    oc, lc = fn(q, k, v, kv_lens)
    fn0 = torch.compile(lambda a, b, c: sageattn_splitkv_compilable(a, b, c, num_splits=3), fullgraph=True)
    o0 = fn0(q, k, v)
    torch.cuda.synchronize()
    assert torch.equal(oe, o) and torch.equal(le, lse) and torch.equal(oc, o) and torch.equal(lc, lse)
    assert torch.equal(o0, sa.sageattn_splitkv(q, k, v, num_splits=3))
    assert torch.equal(o[1], torch.zeros_like(o[1])) and torch.isfinite(o.float()).all()
