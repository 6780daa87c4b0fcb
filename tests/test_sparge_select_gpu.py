"""sage_block_select on the GPU: the TOPK rule, kept key blocks under both rules, and the keywords of sparge_plan /
sageattn_sparge / sageattn_sparge_compilable, against the restated rule of tests/sparge_select_util.py.

The reference takes the pooling kernel's OWN outputs (fp32) and works in fp64, so only the rounding of the selection kernel's
fp32 dot separates the two: on every row that is firm (the k-th and (k+1)-th candidate scores differ by more than the sum of
their bounds, see sparge_select_util) the selected set must be the reference's exactly.  Counts are exact on every row."""
import functools

import pytest
import torch

import sparge_select_util as S
import sparge_util as U

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(name):
    """q, k on the GPU, the library's smoothing mean, the case's fp64 reference (for simthreshd1) and the rule on the
    pooling kernel's outputs."""
    from sageattention_amd import quant
    q, k = U.inputs(name)
    qg, kg = q.cuda(), k.cuda()
    km = quant.k_mean(kg)
    r = U.Ref(name, km.cpu())
    assert r.gap[1] - r.gap[0] >= 0.1, r.gap
    pq, sq = quant.block_pool_sim(qg, 128)
    pk, sk = quant.block_pool_sim(kg, 64, mean=km)
    rule = S.Rule(pq.cpu(), sq.cpu(), pk.cpu(), sk.cpu(), r.sm_scale, r.simthr)
    assert torch.equal(rule.elig, r.elig) and torch.equal(rule.selfsim, r.selfsim)  # no decision near simthreshd1
    return qg, kg, km, r, rule


@functools.lru_cache(maxsize=None)
def predicted(name, rule, param, keeps):
    """-> (plan, bool map on the CPU) of sparge_plan under `rule` ("topk" | "cdf")."""
    import sageattention_amd as sa
    qg, kg, km, r, _ = case(name)
    kw = dict(topk=param) if rule == "topk" else dict(cdfthreshd=param)
    plan, bmap = sa.sparge_plan(qg, kg, simthreshd1=r.simthr, km=km, return_map=True, keep_first=keeps[0],
                                keep_last=keeps[1], **kw)
    return plan, bmap.cpu()


def _v(name, seed=7):
    D, M, N, Hq, Hk, B, dtype = U.CASES[name]
    return torch.randn(B, Hk, N, D, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


# ---- 1. counts, 2. the selected set ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("keeps", S.KEEPS)
@pytest.mark.parametrize("topk", S.TOPKS)
@pytest.mark.parametrize("name", list(U.CASES))
def test_topk_counts_are_exact_and_firm_rows_equal_the_rule(name, topk, keeps):
    _, _, _, _, rule = case(name)
    _, m = predicted(name, "topk", topk, keeps)
    cand = rule.cand(*keeps)
    ss = rule.selfsim.squeeze(-1)
    live = rule.live(cand)
    n, kc = cand.sum(-1), rule.kc(cand, topk)
    assert m[(~cand).expand_as(m)].all()          # kept and ineligible tiles are on in every row
    assert m[~ss].all()                           # rows that are not self-similar are all on
    got = (m & cand).sum(-1)
    print(f"{name} topk {topk} keeps {keeps}: density {float(m.float().mean()):.3f}, n {sorted(set(n.flatten().tolist()))}, "
          f"kcount {sorted(set(kc.flatten().tolist()))}, selected per live row {sorted(set(got[live].tolist()))}")
    assert live.any() and torch.equal(got[live], kc.expand(-1, -1, rule.nqb)[live])
    assert torch.equal(m.sum(-1)[ss], (rule.ntk - n + kc).expand(-1, -1, rule.nqb)[ss])
    firm, _ = rule.firm(cand, topk)
    notfirm = int((live & ~firm).sum())
    print(f"  live rows {int(live.sum())}, not firm {notfirm}")
    assert notfirm <= S.NONFIRM_CAP * int(live.sum())
    assert torch.equal(m[firm], rule.map("topk", topk, *keeps)[firm])


# ---- 3. list format ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,param", [("topk", 0.3), ("cdf", 0.9)])
@pytest.mark.parametrize("name", list(U.CASES))
def test_lists_are_the_compactors(name, rule, param):
    import sageattention_amd as sa
    _, _, _, r, _ = case(name)
    for keeps in S.KEEPS:
        plan, bmap = predicted(name, rule, param, keeps)
        assert (plan.B, plan.Hq, plan.M, plan.N) == (r.B, r.Hq, r.M, r.N)
        assert torch.equal(plan.lists, sa.block_sparse_plan(bmap.cuda(), r.M, r.N).lists)


# ---- 4. the CDF rule through the new entry point ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.CASES))
def test_cdf_without_keeps_is_todays_call(name):
    """sage_block_select(SAGE_SELECT_CDF, keeps 0) and sage_block_select_cdf write the same lists and maps."""
    from sageattention_amd import _lib as L
    from sageattention_amd import quant
    qg, kg, km, r, _ = case(name)
    pq, sq = quant.block_pool_sim(qg, 128)
    pk, sk = quant.block_pool_sim(kg, 64, mean=km)
    thr = torch.full((r.Hq,), r.simthr, dtype=torch.float32, device="cuda")
    lib = L.lib()
    nints = lib.sage_block_sparse_workspace_bytes(r.B, r.Hq, r.M, r.N) // 4
    shape = (r.B, r.Hq, (r.M + 127) // 128, (r.N + 63) // 64)
    for cdf in (0.5, 0.9, 1.0):
        par = torch.full((r.Hq,), cdf, dtype=torch.float32, device="cuda")
        old, new = (torch.full((nints,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        mold, mnew = (torch.full(shape, 9, dtype=torch.uint8, device="cuda") for _ in range(2))
        stats = (pq.data_ptr(), sq.data_ptr(), pk.data_ptr(), sk.data_ptr(), r.B, r.Hq, r.Hk, r.M, r.N, r.D, r.sm_scale,
                 thr.data_ptr())
        L.check(lib.sage_block_select_cdf(*stats, par.data_ptr(), old.data_ptr(), nints * 4, mold.data_ptr(),
                                          L.stream_ptr(qg.device)), "sage_block_select_cdf")
        L.check(lib.sage_block_select(*stats, L.SELECT_CDF, par.data_ptr(), 0, 0, new.data_ptr(), nints * 4, mnew.data_ptr(),
                                      L.stream_ptr(qg.device)), "sage_block_select")
        assert torch.equal(old, new) and torch.equal(mold, mnew), cdf
        plan, bmap = predicted(name, "cdf", cdf, (0, 0))   # ... and so does sparge_plan
        assert torch.equal(plan.lists, old) and torch.equal(bmap, mold.cpu().bool())
        assert bool(bmap.all()) == (cdf == 1.0)


@pytest.mark.parametrize("cdf", U.CDFS)
@pytest.mark.parametrize("name", list(U.CASES))
def test_cdf_with_keeps_selection_properties(name, cdf):
    """The three selection properties of tests/test_sparge_gpu.py over the CANDIDATES, with p the fp64 softmax over them:
    (a) S holds the mass asked for, (b) without its smallest member it would not, (c) S is a top set."""
    _, _, _, _, rule = case(name)
    keeps = (2, 1)
    _, m = predicted(name, "cdf", cdf, keeps)
    cand = rule.cand(*keeps)
    live = rule.live(cand)
    _, p = rule.select_cdf(cand, cdf)
    forced = (~cand | ~rule.selfsim).expand_as(m)
    assert m[forced].all() and m.any(-1).all()
    assert m[..., :2].all() and m[..., -1].all()
    Sel = m & cand & rule.selfsim
    mass = (p * Sel).sum(-1)
    smallest = torch.where(Sel, p, torch.full_like(p, float("inf"))).amin(-1)
    largest_out = torch.where(cand & ~Sel & rule.selfsim, p, torch.zeros_like(p)).amax(-1)
    print(f"{name} cdf {cdf} keeps {keeps}: density {float(m.float().mean()):.3f}, min mass {float(mass[live].min()):.5f}, "
          f"max mass-without-smallest {float((mass - smallest)[live].max()):.5f}")
    assert live.any() and Sel.any(-1)[live].all()
    assert (mass >= cdf - U.DELTA)[live].all()
    assert ((mass - smallest) < cdf + U.DELTA)[live].all()
    assert (smallest >= (1 - 1e-4) * largest_out)[live].all()


# ---- 5. ties ---------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_indices_across_the_lane_step():
    """K with every row the same non-zero vector and km = 0: all 71 pooled key blocks are bit-equal (sums of at most 128
    copies of an fp16 value are exact in fp32, and so is the division), so every score of a row is the same and the lower
    index decides -- over more than one 64-lane step."""
    import sageattention_amd as sa
    qg, _, _, r, rule = case("c2")
    D, M, N, Hq, Hk, B, dtype = U.CASES["c2"]
    assert N == 64 * 70 + 5
    row = torch.randn(D, generator=torch.Generator().manual_seed(5)).to(dtype)
    assert (row != 0).all()
    k = row.view(1, 1, 1, D).expand(B, Hk, N, D).contiguous().cuda()
    km = torch.zeros(B, Hk, D, dtype=dtype, device="cuda")
    ss = rule.selfsim.squeeze(-1)
    assert ss.any()
    ntk = 71
    for keeps, first in (((0, 0), 0), ((2, 1), 2)):
        n = ntk - keeps[0] - keeps[1]
        kc = int(S.kcount(0.95, n))
        assert kc > 64 and kc < n
        _, bmap = sa.sparge_plan(qg, k, simthreshd1=r.simthr, topk=0.95, km=km, return_map=True, keep_first=keeps[0],
                                 keep_last=keeps[1])
        want = torch.zeros(ntk, dtype=torch.bool)
        want[:first + kc] = True
        if keeps[1]:
            want[-keeps[1]:] = True
        m = bmap.cpu()
        assert torch.equal(m[ss], want.expand_as(m)[ss]), keeps
        assert m[~ss].all()


# ---- 6. per-head topk ------------------------------------------------------------------------------------------------------------
def test_per_head_topk_and_determinism():
    import sageattention_amd as sa
    qg, kg, km, r, _ = case("c1")
    vals = [1.0, 0.125, 0.3, 0.5]
    topk = torch.tensor(vals)
    kw = dict(simthreshd1=r.simthr, km=km, keep_first=2, keep_last=1)
    plan, bmap = sa.sparge_plan(qg, kg, topk=topk.cuda(), return_map=True, **kw)
    bmap = bmap.cpu()
    assert bmap[:, 0].all()                                         # a head with 1.0 is all on
    for h in (1, 2, 3):
        assert torch.equal(bmap[:, h], predicted("c1", "topk", vals[h], (2, 1))[1][:, h]), h
    assert not bmap[:, 1].all()
    again = sa.sparge_plan(qg, kg, topk=topk, **kw)                 # a CPU tensor is moved
    assert torch.equal(plan.lists, again.lists)
    ones = sa.sparge_plan(qg, kg, simthreshd1=r.simthr, km=km, topk=1.0, return_map=True)
    full = sa.sparge_plan(qg, kg, simthreshd1=r.simthr, km=km, cdfthreshd=1.0, return_map=True)
    assert torch.equal(ones[1], full[1]) and torch.equal(ones[0].lists, full[0].lists) and bool(ones[1].all())
    with pytest.raises(ValueError, match="shape"):
        sa.sparge_plan(qg, kg, topk=torch.ones(r.Hq + 1))


# ---- 7. the operator -------------------------------------------------------------------------------------------------------------
KW = dict(topk=0.3, keep_first=2, keep_last=1)


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("name", ["c1", "c3bf"])
def test_operator_equals_block_sparse_on_the_predicted_plan(name, pv):
    import sageattention_amd as sa
    qg, kg, _, r, _ = case(name)
    v = _v(name)
    o, lse, plan = sa.sageattn_sparge(qg, kg, v, pv=pv, simthreshd1=r.simthr, return_lse=True, return_plan=True, **KW)
    want = sa.sparge_plan(qg, kg, simthreshd1=r.simthr, **KW)
    assert torch.equal(plan.lists, want.lists)
    assert torch.equal(plan.lists, predicted(name, "topk", 0.3, (2, 1))[0].lists)
    assert not torch.equal(plan.lists, predicted(name, "topk", 0.3, (0, 0))[0].lists)
    o_ref, lse_ref = sa.sageattn_block_sparse(qg, kg, v, want, pv=pv, return_lse=True)
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    assert torch.equal(sa.sageattn_sparge(qg, kg, v, pv=pv, simthreshd1=r.simthr, **KW), o_ref)
    # cdfthreshd is not read when topk is given
    assert torch.equal(sa.sageattn_sparge(qg, kg, v, pv=pv, simthreshd1=r.simthr, cdfthreshd=0.1, **KW), o_ref)


def test_operator_nhd_and_per_warp():
    import sageattention_amd as sa
    qg, kg, _, r, _ = case("c1")
    v = _v("c1")
    kw = dict(simthreshd1=r.simthr, qk_quant_gran="per_warp", return_lse=True, **KW)
    o, lse = sa.sageattn_sparge(qg, kg, v, **kw)
    on, lsen = sa.sageattn_sparge(*(t.transpose(1, 2).contiguous() for t in (qg, kg, v)), tensor_layout="NHD", **kw)
    assert torch.equal(on.transpose(1, 2), o) and torch.equal(lsen, lse)


def test_operator_pads_head_dim_96():
    import sageattention_amd as sa
    g = torch.Generator().manual_seed(96)
    q = U._clustered(1, 2, 300, 96, 128, 4, 0.0, g).half().cuda()
    k = U._clustered(1, 2, 333, 96, 64, 5, 3.0, g).half().cuda()
    v = torch.randn(1, 2, 333, 96, generator=g).half().cuda()
    kw = dict(simthreshd1=0.45, topk=0.5, keep_first=1, keep_last=1)
    plan, bmap = sa.sparge_plan(q, k, return_map=True, **kw)
    pad = lambda t: torch.nn.functional.pad(t, (0, 32))  # noqa: E731
    plan_p = sa.sparge_plan(pad(q), pad(k), sm_scale=96 ** -0.5, **kw)
    assert torch.equal(plan.lists, plan_p.lists) and not bmap.all() and bmap.any(-1).all()
    assert bmap[..., 0].all() and bmap[..., -1].all()
    for pv in ("fp16", "fp8"):
        o, lse = sa.sageattn_sparge(q, k, v, pv=pv, return_lse=True, **kw)
        o_ref, lse_ref = sa.sageattn_block_sparse(q, k, v, plan, pv=pv, return_lse=True)
        assert o.shape == q.shape and torch.equal(o, o_ref) and torch.equal(lse, lse_ref)


# ---- 8. capture and compile --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_operator_captures_into_a_hip_graph(pv):
    import sageattention_amd as sa
    qg, kg, _, r, _ = case("c3")
    q, k, v = qg.clone(), kg.clone(), _v("c3")
    kw = dict(pv=pv, simthreshd1=r.simthr, return_lse=True, **KW)
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


@pytest.mark.parametrize("kw", [dict(topk=0.3), dict(topk=0.3, keep_first=2, keep_last=1), dict(cdfthreshd=0.9, keep_last=1)],
                         ids=["topk", "topk_keeps", "cdf_keeps"])
def test_compiles_as_one_graph(kw):
    import sageattention_amd as sa
    import sageattention_amd.ops as ops
    qg, kg, _, r, _ = case("c1")
    v = _v("c1")

    def block(q, k, v):
        o, lse = ops.sageattn_sparge_compilable(q * 1.0, k, v, simthreshd1=r.simthr, return_lse=True, **kw)
        return o + 1.0, lse

    oc, lc = torch.compile(block, backend="aot_eager", fullgraph=True)(qg, kg, v)
    oe, le = sa.sageattn_sparge(qg, kg, v, simthreshd1=r.simthr, return_lse=True, **kw)
    assert torch.equal(oc, oe + 1.0) and torch.equal(lc, le)
    assert torch.equal(ops.sageattn_sparge_compilable(qg, kg, v, simthreshd1=r.simthr, **kw), oe)
