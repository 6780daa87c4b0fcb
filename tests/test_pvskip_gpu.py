"""The P.V skip of block-sparse attention on the GPU (pvthreshd / return_skipped).  The gate is exactness on inputs whose
every wave-tile is either far below or close to the running maximum (tests/pvskip_util.py, firmness asserted on the CPU in
tests/test_pvskip.py): the counters equal the restatement's, and a wave that skipped tiles produces, bit for bit, what the
kernel without the skip produces on the map with those tiles switched off."""
import math

import pytest
import torch

import pvskip_util as U
from blocksparse_util import make_map

pytestmark = pytest.mark.gpu

THR = 16.0


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    return sageattention_amd


def _dev(*ts):
    return tuple(t.cuda() for t in ts)


# (head_dim, pv, granularity, dtype): FP16 and FP8 PV at both head_dims and granularities, and one bf16 case
FIRM_CASES = [(D, pv, g, torch.float16) for D in (64, 128) for pv in ("fp16", "fp8") for g in ("per_warp", "per_thread")]
FIRM_CASES.append((64, "fp16", "per_thread", torch.bfloat16))
_ids = lambda c: "-".join(str(x).replace("torch.", "") for x in c)  # noqa: E731


def _check_waves_against_switched_off_tiles(sa, q, k, v, bm, skipped, o, lse, pv, gran, heads=None):
    """for each wave index w: the rows of wave w equal the call without pvthreshd on the map without wave w's skipped tiles"""
    M = q.shape[2]
    hs = slice(None) if heads is None else heads
    for w in range(4):
        bm_w = U.map_without(bm, skipped, w)
        o_w, lse_w = sa.sageattn_block_sparse(q, k, v, bm_w.cuda(), pv=pv, qk_quant_gran=gran, return_lse=True)
        rows = U.wave_rows(M, w).cuda()
        assert torch.equal(o[:, hs][:, :, rows], o_w[:, hs][:, :, rows]), f"o of wave {w}"
        assert torch.equal(lse[:, hs][:, :, rows], lse_w[:, hs][:, :, rows]), f"lse of wave {w}"


@pytest.mark.parametrize("case", FIRM_CASES, ids=_ids)
def test_exact_on_firm_inputs(sa, case):
    D, pv, gran, dtype = case
    q, k, v, bm, _, skipped, counts, _, _ = U.firm_case(D, gran, dtype, THR)
    assert counts.sum() > 0
    q, k, v = _dev(q, k, v)
    o, lse, sk = sa.sageattn_block_sparse(q, k, v, bm.cuda(), pv=pv, qk_quant_gran=gran, return_lse=True, pvthreshd=THR,
                                          return_skipped=True)
    torch.cuda.synchronize()
    assert sk.dtype == torch.int32 and tuple(sk.shape) == tuple(counts.shape)
    assert torch.equal(sk.cpu(), counts), (sk.cpu() - counts).nonzero().tolist()
    _check_waves_against_switched_off_tiles(sa, q, k, v, bm, skipped, o, lse, pv, gran)


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("cfg", [(64, "per_thread", 1, 4, 2, 300, 333), (128, "per_warp", 2, 2, 2, 513, 1027)],
                         ids=lambda c: "-".join(map(str, c)))
def test_huge_threshold_equals_no_threshold(sa, pv, cfg):
    """pins the non-skip path of the new kernels to the existing ones: bitwise, counters 0"""
    D, gran, B, Hq, Hk, M, N = cfg
    g = torch.Generator().manual_seed(M + N)
    q, k, v = _dev(*(torch.randn(B, H, n, D, generator=g).half() for H, n in ((Hq, M), (Hk, N), (Hk, N))))
    bm = make_map(B, Hq, M, N, density=0.4, seed=N).cuda()
    o0, l0 = sa.sageattn_block_sparse(q, k, v, bm, pv=pv, qk_quant_gran=gran, return_lse=True)
    per_head = torch.full((Hq,), 1e30)
    per_head[0] = float("inf")
    for thr in (1e30, per_head):
        o, lse, sk = sa.sageattn_block_sparse(q, k, v, bm, pv=pv, qk_quant_gran=gran, return_lse=True, pvthreshd=thr,
                                              return_skipped=True)
        torch.cuda.synchronize()
        assert torch.equal(o, o0) and torch.equal(lse, l0)
        assert int(sk.abs().sum()) == 0


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_per_head_thresholds(sa, pv):
    """tensor([inf, 16]): head 0 is the call without the keyword with counters 0, head 1 as in the exactness test"""
    D, gran = 64, "per_thread"
    q, k, v, bm, logits, _, _, _, _ = U.firm_case(D, gran, torch.float16, THR)
    skipped, counts, _, _ = U.restate(logits, bm, [math.inf, THR])
    assert counts[:, 0].sum() == 0 and counts[:, 1].sum() > 0
    q, k, v = _dev(q, k, v)
    thr = torch.tensor([float("inf"), THR])
    o, lse, sk = sa.sageattn_block_sparse(q, k, v, bm.cuda(), pv=pv, qk_quant_gran=gran, return_lse=True, pvthreshd=thr,
                                          return_skipped=True)
    o0, l0 = sa.sageattn_block_sparse(q, k, v, bm.cuda(), pv=pv, qk_quant_gran=gran, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(sk.cpu(), counts)
    assert torch.equal(o[:, 0], o0[:, 0]) and torch.equal(lse[:, 0], l0[:, 0])
    _check_waves_against_switched_off_tiles(sa, q, k, v, bm, skipped, o, lse, pv, gran, heads=slice(1, 2))


def _ulp(x, dtype):
    """one unit in the last place of `dtype` at |x| (fp32 tensor in, fp32 out)"""
    mant = 10 if dtype == torch.float16 else 7
    tiny = -14 if dtype == torch.float16 else -126
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** tiny)))
    return torch.exp2(e - mant)


@pytest.mark.parametrize("case", [(64, "fp16", "per_thread"), (128, "fp8", "per_warp"), (64, "fp8", "per_thread"),
                                  (128, "fp16", "per_thread")], ids=_ids)
def test_bound_on_inputs_that_are_not_firm(sa, case):
    """Against the call without the keyword, per row, n_s = the wave's reported count:
        |o' - o|     <= 2 n_s 64 e^-thr 1.13 max|v| + one ulp of the output dtype at |o|
        |lse' - lse| <= 2 n_s 64 e^-thr + 1e-5
    The skipped mass delta is at most n_s 64 e^-thr of a row sum that is >= 1; the numerator moves by at most delta max|v|;
    1.13 covers the FP8 rounding of V.  Inputs: tests/pvskip_util.py loose_case -- tiles at the scaled-logit levels
    {0, -12, -24, -36} (key levels twice that, the generator's logit being half the key level), noise 0.5, thr = 20: with
    the levels read as key levels no tile would come within 20 of being skipped and every counter would be 0."""
    D, pv, gran = case
    thr = 20.0
    q, k, v, bm, logits = U.loose_case(D, gran, torch.float16)
    # some wave-tile is certainly skipped, whatever the lag of the kernel's reference maximum; and the inputs are not firm
    _, certain, _, _ = U.restate(logits, bm, thr + U.LAZY[pv])
    _, upper, min_skip, max_keep = U.restate(logits, bm, thr)
    assert certain.sum() > 0 and (min_skip < thr + U.LAZY[pv] + 1 or max_keep > thr - 1)
    q, k, v = _dev(q, k, v)
    o1, l1, sk = sa.sageattn_block_sparse(q, k, v, bm.cuda(), pv=pv, qk_quant_gran=gran, return_lse=True, pvthreshd=thr,
                                          return_skipped=True)
    o0, l0 = sa.sageattn_block_sparse(q, k, v, bm.cuda(), pv=pv, qk_quant_gran=gran, return_lse=True)
    torch.cuda.synchronize()
    sk = sk.cpu()
    assert int(sk.sum()) > 0
    assert (sk >= certain).all() and (sk <= upper).all()  # between the certain skips and those by the true running maximum
    M = q.shape[2]
    n_s = sk.repeat_interleave(32, dim=3).flatten(2)[:, :, :M].double()          # [B,Hq,M]: the count of the row's wave
    delta = 2 * n_s * 64 * math.exp(-thr)
    do = (o1.float() - o0.float()).abs().cpu().double()
    dl = (l1 - l0).abs().cpu().double()
    bound_o = (delta * 1.13 * v.float().abs().max().item()).unsqueeze(-1) + _ulp(o0.float().cpu(), torch.float16).double()
    bound_l = delta + 1e-5
    print(f"\n{case}: skipped {int(sk.sum())} wave-tiles (certain {int(certain.sum())}, at most {int(upper.sum())}); "
          f"max|o'-o| = {do.max():.3e} (bound there {bound_o.flatten()[do.argmax()]:.3e}), "
          f"max|lse'-lse| = {dl.max():.3e} (bound there {bound_l.flatten()[dl.argmax()]:.3e})")
    assert (do <= bound_o).all()
    assert (dl <= bound_l).all()


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_operator_capture_and_compile(sa, pv):
    from sageattention_amd.ops import sageattn_block_sparse_compilable, sageattn_sparge_compilable
    D, gran = 64, "per_thread"
    q, k, v, _, _, _, _, _, _ = U.firm_case(D, gran, torch.float16, THR)
    q, k, v = _dev(q, k, v)
    kw = dict(pv=pv, qk_quant_gran=gran, simthreshd1=0.6, cdfthreshd=0.9)
    # the operator on its own prediction == the block-sparse call on the returned plan with the same threshold
    o, lse, plan, sk = sa.sageattn_sparge(q, k, v, return_lse=True, return_plan=True, pvthreshd=THR, return_skipped=True, **kw)
    o2, lse2, sk2 = sa.sageattn_block_sparse(q, k, v, plan, pv=pv, qk_quant_gran=gran, return_lse=True, pvthreshd=THR,
                                             return_skipped=True)
    torch.cuda.synchronize()
    assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(sk, sk2)
    # the traceable forms, eager
    oe, le, ske = sageattn_sparge_compilable(q, k, v, return_lse=True, pvthreshd=THR, return_skipped=True, **kw)
    assert torch.equal(oe, o) and torch.equal(le, lse) and torch.equal(ske, sk)
    ob, skb = sageattn_block_sparse_compilable(q, k, v, plan, pv=pv, qk_quant_gran=gran, pvthreshd=THR, return_skipped=True)
    assert torch.equal(ob, o) and torch.equal(skb, sk)
    # one HIP-graph capture with replay: no host synchronisation inside the call
    thr_t = torch.full((2,), THR, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sageattn_sparge_compilable(q, k, v, return_lse=True, pvthreshd=thr_t, return_skipped=True, **kw)  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, lg, skg = sageattn_sparge_compilable(q, k, v, return_lse=True, pvthreshd=thr_t, return_skipped=True, **kw)
    og.zero_(); lg.zero_(); skg.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(og, o) and torch.equal(lg, lse) and torch.equal(skg, sk)
    # torch.compile(fullgraph=True)
    fn = torch.compile(lambda a, b, c, t: sageattn_sparge_compilable(a, b, c, return_lse=True, pvthreshd=t,
                                                                     return_skipped=True, **kw), fullgraph=True)
    oc, lc, skc = fn(q, k, v, thr_t)
    torch.cuda.synchronize()
    assert torch.equal(oc, o) and torch.equal(lc, lse) and torch.equal(skc, sk)


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_empty_q_block(sa, pv):
    """o = 0 and lse = -inf on the rows of an empty q-block as without the keyword, and its four counters are 0"""
    D, gran = 128, "per_warp"
    q, k, v, bm, logits, _, _, _, _ = U.firm_case(D, gran, torch.float16, THR)
    bm = bm.clone()
    bm[0, 1, 0] = False
    bm[1, 0, 1] = False
    _, counts, _, _ = U.restate(logits, bm, THR)
    q, k, v = _dev(q, k, v)
    sk = None
    o, lse, sk = sa.sageattn_block_sparse(q, k, v, bm.cuda(), pv=pv, qk_quant_gran=gran, return_lse=True, pvthreshd=THR,
                                          return_skipped=True)
    torch.cuda.synchronize()
    assert (o[0, 1, :128] == 0).all() and (lse[0, 1, :128] == -math.inf).all()
    assert (o[1, 0, 128:] == 0).all() and (lse[1, 0, 128:] == -math.inf).all()
    assert torch.equal(sk.cpu(), counts) and int(sk[0, 1, 0].abs().sum()) == 0 and int(sk[1, 0, 1].abs().sum()) == 0
    assert torch.isfinite(lse[0, 0]).all() and torch.isfinite(o.float()).all()
