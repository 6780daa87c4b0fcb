"""Per-batch key lengths on the block-sparse and Sparge paths, on the GPU (the rule: include/sageattn_hip.h, per-batch key
lengths for block-sparse attention, and the predictor with per-batch key lengths).

The reference for batch b is the existing operator on the slice -- ``sageattn_block_sparse`` (with or without the P.V skip),
``sparge_plan`` or ``block_pool_sim`` on ``q[b:b+1]``, the first len_b keys and the map cut to ceil(len_b / 64) columns, on the
same GPU -- and the comparison is ``torch.equal``: the rule admits no tolerance.  In every case the K and V rows >= len_b hold
NaN, so anything that reads them -- a statistic of the pre-pass or of the pooling, a tile copied by the blind read-ahead and
then consumed, a V row times P = 0 -- shows."""
import pytest
import torch

import blocksparse_util as BU
import sparge_util as SU

pytestmark = pytest.mark.gpu

HQ, HK, M, N = 4, 2, 200, 320
LENS = [320, 257, 256, 65, 1, 0]   # full; one row into the last tile; whole tiles; one row into tile 1; one key; none
NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    import sageattention_amd.ops  # noqa: F401  (registers the ops)
    return sageattention_amd


def _make(B, n, D, dtype=torch.float16, seed=0, m=M, layout="HND"):
    """seeded q, k, v on the GPU; k carries a per-channel offset, so that the smoothing mean matters"""
    g = torch.Generator().manual_seed(1000 * D + n + seed)
    q = torch.randn(B, HQ, m, D, generator=g)
    k = torch.randn(B, HK, n, D, generator=g) + 2.0 * torch.randn(B, HK, 1, D, generator=g)
    v = torch.randn(B, HK, n, D, generator=g)
    q, k, v = (t.to(dtype).cuda() for t in (q, k, v))
    if layout == "NHD":
        q, k, v = (t.transpose(1, 2).contiguous() for t in (q, k, v))
    return q, k, v


def _clamped(lens, n):
    return [min(max(int(x), 0), n) for x in lens]


def _poison(k, v, eff, layout="HND"):
    """NaN into the K and V rows >= len_b"""
    for b, n in enumerate(eff):
        for t in (k, v):
            if t is None:
                continue
            if layout == "HND":
                t[b, :, n:] = float("nan")
            else:
                t[b, n:] = float("nan")


def _keys(t, b, n, layout="HND"):
    return t[b:b + 1, :, :n] if layout == "HND" else t[b:b + 1, :n]


def _maps(B):
    """all-ones; two seeded random maps at density 1/2; a map that leaves q-blocks of the short batches only tiles beyond
    their length (batch 3, 65 keys = 2 tiles: q-block 1 of head 0 has tiles 3 and 4; batch 4, 1 key: q-block 0 of head 1 has
    tile 4; batch 1, 257 keys = all 5 tiles, keeps its tile 4)"""
    nqb, ntk = (M + 127) // 128, (N + 63) // 64
    ones = torch.ones(B, HQ, nqb, ntk, dtype=torch.bool)
    beyond = ones.clone()
    beyond[3, 0, 1] = torch.tensor([False, False, False, True, True])
    beyond[4, 1, 0] = torch.tensor([False, False, False, False, True])
    beyond[1, 2, 1] = torch.tensor([False, False, False, False, True])
    return {"ones": ones, "rand1": BU.make_map(B, HQ, M, N, 0.5, 11), "rand2": BU.make_map(B, HQ, M, N, 0.5, 12), "beyond": beyond}


def _as_tuple(x):
    return x if isinstance(x, tuple) else (x,)


def _references(sa, q, k, v, bm, eff, layout="HND", **kw):
    """per batch the existing operator on the slice and the cut map (None for a batch without keys)"""
    refs = []
    for b, n in enumerate(eff):
        if n == 0:
            refs.append(None)
            continue
        cut = bm[b:b + 1, :, :, :(n + 63) // 64].cuda()
        refs.append(_as_tuple(sa.sageattn_block_sparse(q[b:b + 1], _keys(k, b, n, layout), _keys(v, b, n, layout), cut,
                                                       tensor_layout=layout, **kw)))
    torch.cuda.synchronize()
    return refs


def _assert_matches(out, refs, eff, what=""):
    out = _as_tuple(out)
    for b, n in enumerate(eff):
        if n == 0:
            assert torch.equal(out[0][b], torch.zeros_like(out[0][b])), f"{what} batch {b}: o of a batch without keys"
            for t in out[1:]:
                want = NEG_INF if t.dtype == torch.float32 else 0
                assert torch.equal(t[b], torch.full_like(t[b], want)), f"{what} batch {b}: lse / counters of a batch without keys"
            continue
        assert len(out) == len(refs[b])
        for i, (t, r) in enumerate(zip(out, refs[b])):
            assert not torch.isnan(r.float()).any(), "the reference itself"
            assert torch.equal(t[b:b + 1], r), (f"{what} batch {b} (len {n}), result {i}: differs in "
                                                f"{int((t[b:b + 1] != r).sum())} of {r.numel()} elements")


# ---- 1. block-sparse attention ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gran", ["per_thread", "per_warp"])
@pytest.mark.parametrize("pv,dtype", [("fp16", torch.float16), ("fp16", torch.bfloat16), ("fp8", torch.float16)],
                         ids=["fp16", "bf16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_block_sparse_against_the_slices(sa, D, pv, dtype, gran):
    """N = 320 (five tiles), M = 200 (two q-blocks, the second ragged), lengths that end on and off a tile edge, with
    return_lse; every map once as a map and once as a plan"""
    q, k, v = _make(len(LENS), N, D, dtype)
    _poison(k, v, LENS)
    kv_lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    kw = dict(pv=pv, qk_quant_gran=gran, return_lse=True)
    for name, bm in _maps(len(LENS)).items():
        refs = _references(sa, q, k, v, bm, LENS, **kw)
        plan = sa.block_sparse_plan(bm.cuda(), M, N)
        lists = plan.lists.clone()
        for form, m in (("map", bm.cuda()), ("plan", plan)):
            out = sa.sageattn_block_sparse(q, k, v, m, kv_lens=kv_lens, **kw)
            torch.cuda.synchronize()
            _assert_matches(out, refs, LENS, f"{name} as {form}:")
        assert torch.equal(plan.lists, lists), "the lists are read-only"
        if name == "beyond":  # the emptied rows, by the convention of empty q-blocks
            o, lse = out
            assert torch.equal(o[3, 0, 128:], torch.zeros_like(o[3, 0, 128:])) and (lse[3, 0, 128:] == NEG_INF).all()
            assert torch.equal(o[4, 1, :128], torch.zeros_like(o[4, 1, :128])) and (lse[4, 1, :128] == NEG_INF).all()
            assert torch.isfinite(lse[1, 2, 128:]).all() and torch.isfinite(lse[3, 0, :128]).all()


@pytest.mark.parametrize("D,pv,gran", [(64, "fp16", "per_thread"), (64, "fp8", "per_thread"), (128, "fp16", "per_warp"),
                                       (128, "fp8", "per_thread")])
def test_pv_skip_counters(sa, D, pv, gran):
    """with pvthreshd and return_skipped: o, lse and the counters of every batch equal those of the twin on the slice; the
    counters of the emptied q-blocks and of the batch without keys are 0.  The keys of tile 0 are three times as long as the
    others, so that later tiles are negligible for whole waves and skips do happen."""
    q, k, v = _make(len(LENS), N, D, seed=5)
    k[:, :, :64] *= 3.0
    _poison(k, v, LENS)
    kv_lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    kw = dict(pv=pv, qk_quant_gran=gran, return_lse=True, pvthreshd=0.5, return_skipped=True)
    maps = _maps(len(LENS))
    for name in ("ones", "rand1", "beyond"):
        bm = maps[name]
        refs = _references(sa, q, k, v, bm, LENS, **kw)
        for m in (bm.cuda(), sa.block_sparse_plan(bm.cuda(), M, N)):
            out = sa.sageattn_block_sparse(q, k, v, m, kv_lens=kv_lens, **kw)
            torch.cuda.synchronize()
            _assert_matches(out, refs, LENS, f"{name}:")
        skipped = out[2]
        assert tuple(skipped.shape) == (len(LENS), HQ, 2, 4) and skipped.dtype == torch.int32
        if name == "ones":
            assert int(skipped[:3].sum()) > 0, "the inputs are meant to skip"
        if name == "beyond":
            assert int(skipped[3, 0, 1].sum()) == 0 and int(skipped[4, 1, 0].sum()) == 0 and int(skipped[5].sum()) == 0
    # without return_skipped: the same o and lse
    o2, lse2 = sa.sageattn_block_sparse(q, k, v, maps["beyond"].cuda(), kv_lens=kv_lens, pv=pv, qk_quant_gran=gran,
                                        return_lse=True, pvthreshd=0.5)
    assert torch.equal(o2, out[0]) and torch.equal(lse2, out[1])


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_nhd_head_dim_72(sa, pv):
    q, k, v = _make(len(LENS), N, 72, seed=2, layout="NHD")
    _poison(k, v, LENS, "NHD")
    kv_lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    bm = _maps(len(LENS))["rand1"]
    kw = dict(pv=pv, return_lse=True)
    refs = _references(sa, q, k, v, bm, LENS, layout="NHD", **kw)
    o, lse = sa.sageattn_block_sparse(q, k, v, bm.cuda(), tensor_layout="NHD", kv_lens=kv_lens, **kw)
    torch.cuda.synchronize()
    assert o.shape == q.shape and tuple(lse.shape) == (len(LENS), HQ, M)
    # the batch axis leads in either layout, so the per-batch comparison is the same
    _assert_matches((o, lse), refs, LENS, "NHD:")


def test_lengths_outside_the_range_are_clamped(sa):
    lens = [400, -3, 1 << 30, 64]
    eff = _clamped(lens, N)
    q, k, v = _make(len(lens), N, 64, seed=3)
    _poison(k, v, eff)
    bm = BU.make_map(len(lens), HQ, M, N, 0.5, 13)
    for pv in ("fp16", "fp8"):
        refs = _references(sa, q, k, v, bm, eff, pv=pv, return_lse=True)
        out = sa.sageattn_block_sparse(q, k, v, bm.cuda(), pv=pv, return_lse=True,
                                       kv_lens=torch.tensor(lens, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        _assert_matches(out, refs, eff, pv)


# ---- 2. plan reuse and graph capture ---------------------------------------------------------------------------------------
def test_one_plan_serves_any_lengths(sa):
    first, second = LENS, [1, 320, 65, 0, 256, 257]
    q, k, v = _make(len(LENS), N, 128, seed=4)
    bm = _maps(len(LENS))["rand2"]
    plan = sa.block_sparse_plan(bm.cuda(), M, N)
    lists = plan.lists.clone()
    for lens in (first, second, first):
        kq, vq = k.clone(), v.clone()
        _poison(kq, vq, lens)
        refs = _references(sa, q, kq, vq, bm, lens, pv="fp8", return_lse=True)
        out = sa.sageattn_block_sparse(q, kq, vq, plan, pv="fp8", return_lse=True,
                                       kv_lens=torch.tensor(lens, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        _assert_matches(out, refs, lens, str(lens))
        assert torch.equal(plan.lists, lists)


@pytest.mark.parametrize("pv,thr", [("fp16", None), ("fp8", 0.5)])
def test_graph_capture_reads_the_lengths_at_replay(sa, pv, thr):
    """one captured call, kv_lens overwritten in place, replay: the output of an eager call with the new lengths"""
    first, second = [320, 100, 7], [64, 320, 0]
    q, k, v = _make(3, N, 64, seed=6)
    _poison(k, v, [max(a, b) for a, b in zip(first, second)])
    plan = sa.block_sparse_plan(BU.make_map(3, HQ, M, N, 0.5, 14).cuda(), M, N)
    kv_lens = torch.tensor(first, dtype=torch.int32, device="cuda")
    kw = dict(pv=pv, return_lse=True, pvthreshd=thr, return_skipped=thr is not None)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sa.sageattn_block_sparse(q, k, v, plan, kv_lens=kv_lens, **kw)  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = sa.sageattn_block_sparse(q, k, v, plan, kv_lens=kv_lens, **kw)
    for lens in (second, first):
        kv_lens.copy_(torch.tensor(lens, dtype=torch.int32))
        got[0].fill_(1.0); got[1].zero_()
        graph.replay()
        want = sa.sageattn_block_sparse(q, k, v, plan, kv_lens=torch.tensor(lens, dtype=torch.int32, device="cuda"), **kw)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, want)), lens
        assert torch.isfinite(got[0].float()).all()


# ---- 3. the predictor ------------------------------------------------------------------------------------------------------
PN, PM = 4400, 300                   # 69 key blocks: more than the 64 a wave covers per pass
PLENS = [4400, 4097, 4096, 300, 0]   # ragged last block; one row into block 64; exactly 64 blocks; 5 blocks (ragged); none


def _clustered_qk(D, dtype=torch.float16):
    """the clustered inputs of the predictor's tests (self-similar blocks, every 5th K block noise, K offset +3)"""
    g = torch.Generator().manual_seed(D + PN)
    B = len(PLENS)
    q = SU._clustered(B, HQ, PM, D, 128, 4, 0.0, g).to(dtype).cuda()
    k = SU._clustered(B, HK, PN, D, 64, 5, 3.0, g).to(dtype).cuda()
    return q, k


@pytest.mark.parametrize("D", [64, 128])
def test_pooled_statistics_of_the_valid_blocks(sa, D):
    from sageattention_amd import _lib as L
    from sageattention_amd.quant import block_pool_sim, k_smooth_quant_kvlen
    _, k = _clustered_qk(D)
    _poison(k, None, PLENS)
    kv_lens = torch.tensor(PLENS, dtype=torch.int32, device="cuda")
    km = k_smooth_quant_kvlen(k, kv_lens, "HND", L.GRAN_PER_THREAD, L.ROUND_TRITON)[2]
    pooled, sim = block_pool_sim(k, 64, "HND", mean=km, kv_lens=kv_lens)
    torch.cuda.synchronize()
    for b, n in enumerate(PLENS):
        if n == 0:
            continue
        nb = (n + 63) // 64
        rp, rs = block_pool_sim(k[b:b + 1, :, :n], 64, "HND", mean=km[b:b + 1].contiguous())
        assert torch.isfinite(rp).all() and torch.isfinite(rs).all()
        assert torch.equal(pooled[b:b + 1, :, :nb], rp), f"batch {b} (len {n}): pooled"
        assert torch.equal(sim[b:b + 1, :, :nb], rs), f"batch {b} (len {n}): sim"
    # 128-row blocks (the Q geometry) take lengths as well
    pooled, sim = block_pool_sim(k, 128, "HND", mean=km, kv_lens=kv_lens)
    rp, rs = block_pool_sim(k[3:4, :, :300], 128, "HND", mean=km[3:4].contiguous())
    assert torch.equal(pooled[3:4, :, :3], rp) and torch.equal(sim[3:4, :, :3], rs)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_full_lengths_take_the_other_branch_of_one_text(sa, D, dtype):
    """The kernels with and without lengths are the two branches of one text (template flag KVLEN, sage_sparge.hip): with every
    length equal to N they give the same bits -- pooled, sim, lists and map, both block sizes, both rules."""
    from sageattention_amd.quant import block_pool_sim, k_mean
    q, k = _clustered_qk(D, dtype)
    full = torch.full((len(PLENS),), PN, dtype=torch.int32, device="cuda")
    km = k_mean(k, "HND")
    for blk in (64, 128):
        for mean in (None, km):
            got, want = block_pool_sim(k, blk, "HND", mean=mean, kv_lens=full), block_pool_sim(k, blk, "HND", mean=mean)
            assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all()
            assert torch.equal(got[0], want[0]), f"pooled, {blk}-row blocks"
            assert torch.equal(got[1], want[1]), f"sim, {blk}-row blocks"
    for select in (dict(cdfthreshd=0.9), dict(topk=0.25, keep_first=1, keep_last=2)):
        plan, bmap = sa.sparge_plan(q, k, kv_lens=full, return_map=True, **select)
        rplan, rmap = sa.sparge_plan(q, k, return_map=True, **select)
        assert torch.equal(plan.lists, rplan.lists) and torch.equal(bmap, rmap), select
        assert not bmap.all() and bmap.any(), "the inputs are meant to give sparse lists"


@pytest.mark.parametrize("select", [dict(cdfthreshd=0.9), dict(topk=0.25, keep_first=1, keep_last=2)], ids=["cdf", "topk"])
@pytest.mark.parametrize("D", [64, 128])
def test_plan_equals_the_plan_of_the_slice(sa, D, select):
    q, k = _clustered_qk(D)
    _poison(k, None, PLENS)
    kv_lens = torch.tensor(PLENS, dtype=torch.int32, device="cuda")
    plan, bmap = sa.sparge_plan(q, k, kv_lens=kv_lens, return_map=True, **select)
    torch.cuda.synchronize()
    nqb, ntk = (PM + 127) // 128, (PN + 63) // 64
    assert (plan.B, plan.Hq, plan.M, plan.N) == (len(PLENS), HQ, PM, PN) and tuple(bmap.shape) == (len(PLENS), HQ, nqb, ntk)
    lists = plan.lists.view(len(PLENS), HQ, nqb, -1)
    sparse_rows = 0
    for b, n in enumerate(PLENS):
        nb = (n + 63) // 64
        assert not bmap[b, :, :, nb:].any(), f"batch {b}: map columns >= ntk_b"
        if n == 0:
            assert (lists[b, :, :, 0] == 0).all(), "a batch without keys: every list is empty"
            continue
        rplan, rmap = sa.sparge_plan(q[b:b + 1], k[b:b + 1, :, :n], return_map=True, **select)
        rl = rplan.lists.view(1, HQ, nqb, -1)
        assert torch.equal(lists[b, :, :, 0], rl[0, :, :, 0]), f"batch {b} (len {n}): counts"
        assert torch.equal(bmap[b, :, :, :nb], rmap[0]), f"batch {b} (len {n}): map"
        for h in range(HQ):
            for i in range(nqb):
                c = int(rl[0, h, i, 0])
                assert 1 <= c <= nb and torch.equal(lists[b, h, i, 1:1 + c], rl[0, h, i, 1:1 + c]), (b, h, i)
                sparse_rows += c < nb
        if "keep_last" in select:  # keep_last pins the last VALID blocks, keep_first the first
            assert bmap[b, :, :, 0].all() and bmap[b, :, :, max(nb - 2, 0):nb].all()
    assert sparse_rows > 0, "the inputs are meant to give sparse lists"


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_sparge_equals_block_sparse_on_its_plan(sa, D, pv):
    """the 69-block lists through the attention kernels of both head dims"""
    q, k = _clustered_qk(D)
    v = torch.randn(k.shape, generator=torch.Generator().manual_seed(9)).to(k.dtype).cuda()
    _poison(k, v, PLENS)
    kv_lens = torch.tensor(PLENS, dtype=torch.int32, device="cuda")
    kw = dict(topk=0.25, keep_first=1, keep_last=2)
    o, lse, plan = sa.sageattn_sparge(q, k, v, pv=pv, return_lse=True, return_plan=True, kv_lens=kv_lens, **kw)
    want = sa.sparge_plan(q, k, kv_lens=kv_lens, **kw)
    ro, rlse = sa.sageattn_block_sparse(q, k, v, want, pv=pv, return_lse=True, kv_lens=kv_lens)
    torch.cuda.synchronize()
    assert torch.equal(plan.lists, want.lists)
    assert torch.equal(o, ro) and torch.equal(lse, rlse)
    assert torch.isfinite(o[:4].float()).all() and torch.equal(o[4], torch.zeros_like(o[4])) and (lse[4] == NEG_INF).all()
    # ... and, per batch, the existing operator on the slice
    for b, n in ((1, 4097), (3, 300)):
        so, sl = sa.sageattn_sparge(q[b:b + 1], k[b:b + 1, :, :n], v[b:b + 1, :, :n], pv=pv, return_lse=True, **kw)
        assert torch.equal(o[b:b + 1], so) and torch.equal(lse[b:b + 1], sl), (b, n)


# ---- 4. full lengths, torch.compile ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_full_lengths_change_nothing(sa, D, pv):
    q, k, v = _make(3, N, D, seed=7)
    full = torch.full((3,), N, dtype=torch.int32, device="cuda")
    bm = BU.make_map(3, HQ, M, N, 0.5, 15).cuda()
    for kw in (dict(), dict(pvthreshd=0.5, return_skipped=True)):
        a = sa.sageattn_block_sparse(q, k, v, bm, pv=pv, return_lse=True, kv_lens=full, **kw)
        b = sa.sageattn_block_sparse(q, k, v, bm, pv=pv, return_lse=True, **kw)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    a = sa.sageattn_sparge(q, k, v, pv=pv, return_lse=True, kv_lens=full)
    b = sa.sageattn_sparge(q, k, v, pv=pv, return_lse=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("return_lse", [False, True])
@pytest.mark.parametrize("thr", [None, 0.5])
def test_compile_fullgraph(sa, return_lse, thr):
    """the wrappers trace without a graph break and the ops give what the eager operators give"""
    from sageattention_amd.ops import sageattn_block_sparse_compilable, sageattn_sparge_compilable
    lens = [320, 130, 0]
    q, k, v = _make(3, N, 64, seed=8)
    _poison(k, v, lens)
    kv_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    kw = dict(pv="fp8", pvthreshd=thr, return_skipped=thr is not None)
    want = _as_tuple(sa.sageattn_sparge(q, k, v, return_lse=return_lse, kv_lens=kv_lens, **kw))
    fn = torch.compile(lambda a, b, c, n: sageattn_sparge_compilable(a, b, c, return_lse=return_lse, kv_lens=n, **kw),
                       fullgraph=True, backend="aot_eager")
    got = _as_tuple(fn(q, k, v, kv_lens))
    torch.cuda.synchronize()
    assert len(got) == len(want) and all(torch.equal(x, y) for x, y in zip(got, want))
    if not return_lse:  # the block-sparse wrapper has no return_lse: map and plan
        bm = BU.make_map(3, HQ, M, N, 0.5, 16).cuda()
        plan = sa.block_sparse_plan(bm, M, N)
        want = _as_tuple(sa.sageattn_block_sparse(q, k, v, plan, kv_lens=kv_lens, **kw))
        for m in (bm, plan):
            fn = torch.compile(lambda a, b, c, n: sageattn_block_sparse_compilable(a, b, c, m, kv_lens=n, **kw), fullgraph=True,
                               backend="aot_eager")
            got = _as_tuple(fn(q, k, v, kv_lens))
            torch.cuda.synchronize()
            assert len(got) == len(want) and all(torch.equal(x, y) for x, y in zip(got, want))
