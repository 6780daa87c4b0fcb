"""The block-map predictor on the GPU (sage_block_pool_sim, sage_block_select_cdf, sparge_plan, sageattn_sparge) against the
fp64 restatement of its rule in tests/sparge_util.py, on the clustered inputs whose conditions tests/test_sparge.py checks.

Tolerances of the block statistics, u = 2^-24, c = rows of the block (derived from the kernel's summation order, which is
never deeper than the plain sequential one the bounds assume):
  pooled  x' = x - mean rounds once (u), a channel's sum over c rows passes at most c - 1 additions, the division rounds
          once: |d pooled_d| <= (c + 1) u mean_r |x'_rd| <= (c + 2) u mean_r |x'_rd|.
  sim     a squared norm is a sum of positive terms no deeper than 12 operations (8 fmas in a lane, 4 lane steps) and the
          square root halves its relative error; with x', the reciprocal square root and the product each unit component is
          within 10 u; the sum of unit rows adds at most c - 1 roundings: |dS|_2 <= (c + 9) u c, |S| <= c, so
          d(|S|^2 / c^2) <= 2 (c + 9) u; the final sum of D squares (<= 9 operations deep) and the division add 10 u on a value
          <= 1: |d sim| <= (2c + 28) u <= (2c + D + 16) u."""
import functools

import pytest
import torch

import sparge_util as U
import view_cases as V

pytestmark = pytest.mark.gpu
u = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def case(name):
    """The case's q, k on the GPU, the smoothing mean the library computes for k, and the fp64 reference made with it."""
    from sageattention_amd import quant
    q, k = U.inputs(name)
    qg, kg = q.cuda(), k.cuda()
    km = quant.k_mean(kg)
    r = U.Ref(name, km.cpu())
    assert r.gap[1] - r.gap[0] >= 0.1, r.gap
    return qg, kg, km, r


@functools.lru_cache(maxsize=None)
def predicted(name, cdf):
    import sageattention_amd as sa
    qg, kg, _, r = case(name)
    plan, bmap = sa.sparge_plan(qg, kg, simthreshd1=r.simthr, cdfthreshd=cdf, return_map=True)
    return plan, bmap


def _v(name, seed=7):
    D, M, N, Hq, Hk, B, dtype = U.CASES[name]
    return torch.randn(B, Hk, N, D, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


# ---- 5. block statistics ----------------------------------------------------------------------------------------------------
def _check_stats(x_cpu, blk, mean_cpu, pooled, sim, what):
    B, H, n, D = x_cpu.shape
    ref_pooled, ref_sim = U.pool_sim(x_cpu, blk, mean_cpu)
    xa = x_cpu.double() - (mean_cpu.double().unsqueeze(2) if mean_cpu is not None else 0.0)
    nb = (n + blk - 1) // blk
    cnt = torch.full((nb,), float(blk), dtype=torch.float64)
    cnt[-1] = n - (nb - 1) * blk
    mean_abs = torch.stack([xa[:, :, i * blk:(i + 1) * blk].abs().mean(2) for i in range(nb)], 2)
    dp = (pooled.cpu().double() - ref_pooled).abs()
    tol_p = (cnt.view(1, 1, nb, 1) + 2) * u * mean_abs
    ds = (sim.cpu().double() - ref_sim).abs()
    tol_s = (2 * cnt.view(1, 1, nb) + D + 16) * u
    print(f"{what}: max |d pooled| / tol = {float((dp / tol_p).max()):.3f}, max |d sim| = {float(ds.max()):.3e} "
          f"(tol {float(tol_s.min()):.3e})")
    assert pooled.shape == ref_pooled.shape and sim.shape == ref_sim.shape
    assert (dp <= tol_p).all(), (what, float((dp / tol_p).max()))
    assert (ds <= tol_s).all(), (what, float(ds.max()))


@pytest.mark.parametrize("name", list(U.CASES))
def test_block_statistics(name):
    from sageattention_amd import quant
    qg, kg, km, r = case(name)
    pq, sq = quant.block_pool_sim(qg, 128)
    _check_stats(r.q, 128, None, pq, sq, f"{name} q")
    pk, sk = quant.block_pool_sim(kg, 64, mean=km)
    _check_stats(r.k, 64, r.km, pk, sk, f"{name} k - km")
    pk0, sk0 = quant.block_pool_sim(kg, 64)
    _check_stats(r.k, 64, None, pk0, sk0, f"{name} k")
    # dropping km would be seen: without it every K block looks self-similar on these inputs
    assert sk0.min() > 0.85 and sk.min() < 0.3
    # both block lengths on both tensors
    pk128, sk128 = quant.block_pool_sim(kg, 128, mean=km)
    _check_stats(r.k, 128, r.km, pk128, sk128, f"{name} k - km, blk 128")
    pq64, sq64 = quant.block_pool_sim(qg, 64)
    _check_stats(r.q, 64, None, pq64, sq64, f"{name} q, blk 64")


def test_block_statistics_nhd_and_strided_view():
    """The same statistics from an NHD tensor and from a view that slices heads and batches out of poisoned memory."""
    from sageattention_amd import quant
    qg, kg, km, r = case("c1")
    want = quant.block_pool_sim(kg, 64, mean=km)
    got = quant.block_pool_sim(kg.transpose(1, 2).contiguous(), 64, "NHD", mean=km)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for kind in ("head_batch_slice", "seq_slice_nhd"):
        view = V.make_input(kind, values=r.k, seed=3).to("cuda")
        got = quant.block_pool_sim(view.arg(), 64, view.layout, mean=km)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), kind
        assert view.parent_unchanged()


# ---- 6. selection properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdf", U.CDFS)
@pytest.mark.parametrize("name", list(U.CASES))
def test_selection_properties(name, cdf):
    """With p of the fp64 rule and S = the kernel's selected eligible tiles, on every row in which a selection takes place:
    (a) S holds the mass asked for, (b) without its smallest member it would not (the shortest prefix; an all-ones map fails
    this), (c) S is a top set.  Forced tiles equal the rule's exactly, and so does the whole map of every row whose selection
    does not flip within cdfthreshd +- DELTA."""
    _, _, _, r = case(name)
    plan, bmap = predicted(name, cdf)
    m = bmap.cpu()
    forced = (~r.elig | ~r.selfsim).expand_as(m)
    assert m[forced].all()
    assert m.any(-1).all()
    S = m & r.elig & r.selfsim
    live = r.live
    mass = (r.p * S).sum(-1)
    smallest = torch.where(S, r.p, torch.full_like(r.p, float("inf"))).amin(-1)
    largest_out = torch.where(r.elig & ~S & r.selfsim, r.p, torch.zeros_like(r.p)).amax(-1)
    print(f"{name} cdf {cdf}: density {float(m.float().mean()):.3f}, min mass {float(mass[live].min()):.5f}, "
          f"max mass-without-smallest {float((mass - smallest)[live].max()):.5f}")
    assert S.any(-1)[live].all()
    assert (mass >= cdf - U.DELTA)[live].all()
    assert ((mass - smallest) < cdf + U.DELTA)[live].all()
    assert (smallest >= (1 - 1e-4) * largest_out)[live].all()
    if cdf in (0.5, 0.9):
        firm = ~r.marginal(cdf)
        assert torch.equal(m[firm], r.map(cdf)[firm])


# ---- 7. list format ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdf", U.CDFS + (1.0,))
@pytest.mark.parametrize("name", list(U.CASES))
def test_lists_are_the_compactors(name, cdf):
    import sageattention_amd as sa
    _, _, _, r = case(name)
    plan, bmap = predicted(name, cdf)
    assert (plan.B, plan.Hq, plan.M, plan.N) == (r.B, r.Hq, r.M, r.N)
    assert torch.equal(plan.lists, sa.block_sparse_plan(bmap, r.M, r.N).lists)
    if cdf == 1.0:
        assert bmap.all()


# ---- 8. the operator -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("name", ["c1", "c3bf"])
def test_operator_equals_block_sparse_on_the_predicted_plan(name, pv):
    import sageattention_amd as sa
    qg, kg, _, r = case(name)
    v = _v(name)
    kw = dict(simthreshd1=r.simthr, cdfthreshd=0.9)
    o, lse, plan = sa.sageattn_sparge(qg, kg, v, pv=pv, return_lse=True, return_plan=True, **kw)
    want = sa.sparge_plan(qg, kg, **kw)
    assert torch.equal(plan.lists, want.lists)
    assert not torch.equal(plan.lists, predicted(name, 1.0)[0].lists)  # a sparse plan
    o_ref, lse_ref = sa.sageattn_block_sparse(qg, kg, v, want, pv=pv, return_lse=True)
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    assert torch.equal(sa.sageattn_sparge(qg, kg, v, pv=pv, **kw), o_ref)
    # cdfthreshd = 1: every tile
    ones = torch.ones(1, 1, (r.M + 127) // 128, (r.N + 63) // 64, dtype=torch.bool, device="cuda")
    o1, lse1 = sa.sageattn_sparge(qg, kg, v, pv=pv, simthreshd1=r.simthr, cdfthreshd=1.0, return_lse=True)
    o1_ref, lse1_ref = sa.sageattn_block_sparse(qg, kg, v, ones, pv=pv, return_lse=True)
    assert torch.equal(o1, o1_ref) and torch.equal(lse1, lse1_ref)


def test_operator_nhd_and_per_warp():
    import sageattention_amd as sa
    qg, kg, _, r = case("c1")
    v = _v("c1")
    kw = dict(simthreshd1=r.simthr, cdfthreshd=0.9, qk_quant_gran="per_warp", return_lse=True)
    o, lse = sa.sageattn_sparge(qg, kg, v, **kw)
    on, lsen = sa.sageattn_sparge(*(t.transpose(1, 2).contiguous() for t in (qg, kg, v)), tensor_layout="NHD", **kw)
    assert torch.equal(on.transpose(1, 2), o) and torch.equal(lsen, lse)


def test_operator_pads_head_dim_96():
    """Zero padding changes neither dot products nor norms: the plan of a head_dim-96 input is the plan of the same input
    padded by hand, and the operator equals the block-sparse operator on it."""
    import sageattention_amd as sa
    g = torch.Generator().manual_seed(96)
    q = U._clustered(1, 2, 300, 96, 128, 4, 0.0, g).half().cuda()
    k = U._clustered(1, 2, 333, 96, 64, 5, 3.0, g).half().cuda()
    v = torch.randn(1, 2, 333, 96, generator=g).half().cuda()
    kw = dict(simthreshd1=0.45, cdfthreshd=0.9)
    plan, bmap = sa.sparge_plan(q, k, return_map=True, **kw)
    pad = lambda t: torch.nn.functional.pad(t, (0, 32))  # noqa: E731
    plan_p = sa.sparge_plan(pad(q), pad(k), sm_scale=96 ** -0.5, **kw)
    assert torch.equal(plan.lists, plan_p.lists) and not bmap.all() and bmap.any(-1).all()
    for pv in ("fp16", "fp8"):
        o, lse = sa.sageattn_sparge(q, k, v, pv=pv, return_lse=True, **kw)
        o_ref, lse_ref = sa.sageattn_block_sparse(q, k, v, plan, pv=pv, return_lse=True)
        assert o.shape == q.shape and torch.equal(o, o_ref) and torch.equal(lse, lse_ref)


# ---- 9. thresholds and determinism -------------------------------------------------------------------------------------------------
def test_per_head_thresholds_and_determinism():
    import sageattention_amd as sa
    qg, kg, km, r = case("c1")
    cdf = torch.tensor([1.0] + [0.5] * (r.Hq - 1))
    thr = torch.full((r.Hq,), r.simthr)
    plan, bmap = sa.sparge_plan(qg, kg, simthreshd1=thr, cdfthreshd=cdf.cuda(), return_map=True)
    assert bmap[:, 0].all()
    assert torch.equal(bmap[:, 1:], predicted("c1", 0.5)[1][:, 1:])
    # a per-head similarity threshold above every value: nothing is eligible or self-similar in that head, so all is on
    thr2 = thr.clone()
    thr2[1] = 2.0
    _, bmap2 = sa.sparge_plan(qg, kg, simthreshd1=thr2, cdfthreshd=0.5, return_map=True)
    assert bmap2[:, 1].all() and torch.equal(bmap2[:, 2:], predicted("c1", 0.5)[1][:, 2:])
    again = sa.sparge_plan(qg, kg, simthreshd1=thr, cdfthreshd=cdf.cuda(), km=km)
    assert torch.equal(plan.lists, again.lists)
    with pytest.raises(ValueError, match="shape"):
        sa.sparge_plan(qg, kg, cdfthreshd=torch.ones(r.Hq + 1))


# ---- 10. capture and compile ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_operator_captures_into_a_hip_graph(pv):
    import sageattention_amd as sa
    qg, kg, _, r = case("c3")
    q, k, v = qg.clone(), kg.clone(), _v("c3")
    kw = dict(pv=pv, simthreshd1=r.simthr, cdfthreshd=0.9, return_lse=True)
    for _ in range(2):
        sa.sageattn_sparge(q, k, v, **kw)  # warm up: module load, function attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o_g, l_g = sa.sageattn_sparge(q, k, v, **kw)
    for step in (1, 2):  # other values: the batches swapped, then the heads rotated as well
        q.copy_(qg.flip(0) if step == 1 else qg.roll(1, 1))
        k.copy_(kg.flip(0) if step == 1 else kg.roll(1, 1))
        g.replay()
        torch.cuda.synchronize()
        o_e, l_e = sa.sageattn_sparge(q, k, v, **kw)
        assert torch.equal(o_g, o_e) and torch.equal(l_g, l_e)


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_compiles_as_one_graph(pv):
    import sageattention_amd as sa
    import sageattention_amd.ops as ops
    qg, kg, _, r = case("c1")
    v = _v("c1")

    def block(q, k, v):
        o, lse = ops.sageattn_sparge_compilable(q * 1.0, k, v, pv=pv, simthreshd1=r.simthr, cdfthreshd=0.9, return_lse=True)
        return o + 1.0, lse

    oc, lc = torch.compile(block, backend="aot_eager", fullgraph=True)(qg, kg, v)
    oe, le = sa.sageattn_sparge(qg, kg, v, pv=pv, simthreshd1=r.simthr, cdfthreshd=0.9, return_lse=True)
    assert torch.equal(oc, oe + 1.0) and torch.equal(lc, le)
