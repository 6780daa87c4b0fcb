"""sage_block_select (the TOPK rule and kept key blocks of the block-map predictor) without a GPU: the entry point checks
every argument before its first launch, the Python keywords and the new custom ops are in place, the torch restatement of
the rule (tests/sparge_select_util.py) is sound, and the clustered inputs of tests/sparge_util.py meet the condition under
which tests/test_sparge_select_gpu.py may compare the fp32 kernel with the fp64 rule exactly."""
import pytest
import torch

import sparge_select_util as S
import sparge_util as U

# ---- 1. every argument is checked before the first launch ----------------------------------------------------------------
# Fake device addresses, as in tests/test_sparge.py: only where no GPU is visible; there every launch attempt returns
# SAGE_ERR_LAUNCH (-5), which makes a launch observable.
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")

FAKE = 1 << 20
ODD = FAKE + 8
_PARAMS = "pq sq pk sk B Hq Hk M N D sm thr rule par kf kl lists nbytes map stream"


def _valid():
    from sageattention_amd import _lib as L
    B, Hq, M, N = 1, 2, 200, 333
    return dict(pq=FAKE, sq=FAKE, pk=FAKE, sk=FAKE, B=B, Hq=Hq, Hk=1, M=M, N=N, D=64, sm=0.125, thr=FAKE, rule=1, par=FAKE,
                kf=2, kl=1, lists=FAKE, nbytes=L.lib().sage_block_sparse_workspace_bytes(B, Hq, M, N), map=None, stream=None)


def _call(**change):
    from sageattention_amd import _lib as L
    args = dict(_valid(), **change)
    return L.lib().sage_block_select(*[args[n] for n in _PARAMS.split()])


@no_gpu
def test_valid_calls_reach_a_launch():
    assert _call() == -5
    assert _call(rule=0, kf=0, kl=0) == -5
    assert _call(rule=0) == -5 and _call(kf=0, kl=0) == -5
    assert _call(map=FAKE + 1) == -5  # the map is bytes: no alignment asked
    assert _call(N=2048 * 64, nbytes=1 << 40) == -5  # the largest N the LDS row holds
    assert _call(kf=4, kl=3) == -5 and _call(kf=1 << 30, kl=1 << 30) == -5  # 6 key tiles: keep_first + keep_last > ntk
    assert _call(D=128) == -5


@no_gpu
def test_single_fault_status_table():
    """Each argument made invalid on its own returns its argument status: nothing was launched (a launch returns -5 here).
    Every fault sage_block_select_cdf refuses, and the new arguments' own."""
    from sageattention_amd import _lib as L
    need = _valid()["nbytes"]
    cases = [(c, -1) for c in (
        dict(pq=None), dict(pq=ODD), dict(sq=None), dict(pk=None), dict(pk=ODD), dict(sk=None), dict(thr=None),
        dict(lists=None), dict(lists=ODD), dict(nbytes=need - 4), dict(nbytes=0), dict(B=0), dict(Hq=0), dict(Hk=0),
        dict(Hq=3, Hk=2), dict(M=0), dict(N=0), dict(sm=0.0), dict(sm=-1.0), dict(sm=float("nan")), dict(sm=float("inf")),
        dict(nbytes=L.lib().sage_block_sparse_workspace_bytes(1, 2, 200, 64)),  # sized for fewer keys than the call has
        dict(rule=2), dict(rule=-1), dict(par=None), dict(kf=-1), dict(kl=-1))]
    cases += [(dict(D=96), -2), (dict(N=2048 * 64 + 1, nbytes=1 << 40), -4), (dict(N=1 << 25, nbytes=1 << 40), -4)]
    for rule in (0, 1):
        wrong = [(rule, sorted(c), st, got) for c, st in cases if (got := _call(**dict(dict(rule=rule), **c))) != st]
        assert not wrong, wrong


def test_python_errors_and_exports():
    import inspect
    import sageattention_amd as sa
    import sageattention_amd.ops as ops
    from sageattention_amd import _lib as L
    assert {"sageattn_sparge", "sparge_plan"} <= set(sa.__all__) and "sageattn_sparge_compilable" in ops.__all__
    assert "sage_block_select" in L.SIGNATURES and (L.SELECT_CDF, L.SELECT_TOPK) == (0, 1)
    for fn in (sa.sparge_plan, sa.sageattn_sparge, ops.sageattn_sparge_compilable):
        par = inspect.signature(fn).parameters
        assert (par["topk"].default, par["keep_first"].default, par["keep_last"].default) == (None, 0, 0), fn
    # no existing default or position changed
    assert list(inspect.signature(sa.sparge_plan).parameters)[:8] == [
        "q", "k", "tensor_layout", "simthreshd1", "cdfthreshd", "sm_scale", "km", "return_map"]
    assert list(inspect.signature(sa.sageattn_sparge).parameters)[:11] == [
        "q", "k", "v", "tensor_layout", "simthreshd1", "cdfthreshd", "sm_scale", "pv", "qk_quant_gran", "return_lse",
        "return_plan"]
    q = torch.zeros(1, 2, 300, 64, dtype=torch.float16)
    calls = (lambda **kw: sa.sparge_plan(q, q, **kw), lambda **kw: sa.sageattn_sparge(q, q, q, **kw),
             lambda **kw: ops.sageattn_sparge_compilable(q, q, q, **kw))
    for call in calls:
        for kw, word in ((dict(topk=0.0), "topk"), (dict(topk=float("nan")), "topk"), (dict(topk=-0.5), "topk"),
                         (dict(keep_first=-1), "keep_first"), (dict(keep_last=1.5), "keep_last"),
                         (dict(topk=0.3, keep_first=True), "keep_first")):
            with pytest.raises(ValueError, match=word):
                call(**kw)
    for call in calls[:2]:  # valid keywords: the same assertion as without them
        with pytest.raises(AssertionError, match="cuda"):
            call(topk=0.3, keep_first=2, keep_last=1)
        with pytest.raises(AssertionError, match="cuda"):
            call(topk=torch.full((2,), 0.3), keep_last=5)


def _params(schema):
    return str(schema).replace("SymInt", "int")  # torch spells an int argument of a custom op SymInt


def test_op_schemas_and_fake_shapes():
    import sageattention_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    ns = torch.ops.sageattention_amd
    new = ("Tensor q, Tensor k, Tensor v, Tensor simthreshd1, Tensor rule_param, str rule, int keep_first, int keep_last, "
           "str tensor_layout, float sm_scale, str pv, str qk_quant_gran")
    assert f"({new}) -> Tensor" in _params(ns.attn_sparge_select.default._schema)
    assert f"({new}) -> (Tensor, Tensor)" in _params(ns.attn_sparge_select_lse.default._schema)
    old = ("Tensor q, Tensor k, Tensor v, Tensor simthreshd1, Tensor cdfthreshd, str tensor_layout, float sm_scale, str pv, "
           "str qk_quant_gran")
    assert f"({old}) -> Tensor" in str(ns.attn_sparge.default._schema)
    assert f"({old}) -> (Tensor, Tensor)" in str(ns.attn_sparge_lse.default._schema)
    with FakeTensorMode():
        for layout, shp, kshp in (("HND", (2, 8, 300, 96), (2, 4, 333, 96)), ("NHD", (2, 300, 8, 96), (2, 333, 4, 96))):
            q = torch.empty(shp, dtype=torch.bfloat16, device="cuda")
            k = torch.empty(kshp, dtype=torch.bfloat16, device="cuda")
            for kw in (dict(topk=0.3), dict(topk=0.3, keep_first=2, keep_last=1), dict(keep_last=1),
                       dict(topk=torch.empty(8, device="cuda"))):
                o, lse = ops.sageattn_sparge_compilable(q, k, k, tensor_layout=layout, pv="fp8", return_lse=True, **kw)
                assert o.shape == q.shape and o.dtype == q.dtype and o.device == q.device and o.is_contiguous()
                assert lse.shape == (2, 8, 300) and lse.dtype == torch.float32
                o = ops.sageattn_sparge_compilable(q, k, k, tensor_layout=layout, **kw)
                assert o.shape == q.shape and o.dtype == q.dtype and o.is_contiguous()


# ---- 2. the restatement checks itself -------------------------------------------------------------------------------------
def test_kcount_by_hand():
    # float32(0.1) * 50 = 5.00000007... rounds to 5.0f: ceil 5, not 6.  float32(0.3) * 8 = 2.4000001: 3.
    pairs = [(0.1, 50, 5), (0.3, 8, 3), (1e-9, 57, 1), (0.5, 7, 4), (0.125, 56, 7), (0.95, 71, 68), (0.95, 68, 65),
             (0.999, 3, 3), (0.25, 1, 1), (0.0, 9, 1), (-1.0, 9, 1), (0.3, 0, 0)]
    for n in (1, 9, 71):
        pairs += [(1.0, n, n), (1.5, n, n), (float("nan"), n, n), (float("inf"), n, n)]
    wrong = [(t, n, k, got) for t, n, k in pairs if (got := int(S.kcount(t, n))) != k]
    assert not wrong, wrong
    # per head, broadcast against the counts
    k = S.kcount(torch.tensor([0.5, 1.0, float("nan")]).view(1, 3, 1), torch.tensor([[[7]], [[10]]]).expand(2, 3, 1))
    assert k.tolist() == [[[4], [7], [7]], [[5], [10], [10]]]


def test_kept_blocks():
    assert S.kept(6, 0, 0).tolist() == [False] * 6
    assert S.kept(6, 2, 1).tolist() == [True, True, False, False, False, True]
    assert S.kept(6, 9, 0).all() and S.kept(6, 0, 7).all() and S.kept(6, 4, 3).all()  # beyond ntk: as ntk; overlapping


def test_topk_ties_go_to_the_lower_index_and_zeros_are_equal():
    pq = torch.zeros(1, 1, 1, 64, dtype=torch.float64)
    pq[..., 0] = 1.0
    pk = torch.zeros(1, 1, 6, 64, dtype=torch.float64)
    pk[0, 0, :, 0] = torch.tensor([0.1, 0.2, 0.2, 0.2, 0.2, 0.1])
    ones = torch.ones(1, 1, 6, dtype=torch.float64)
    r = S.Rule(pq, ones[..., :1], pk, ones, 1.0, 0.5)
    assert r.select_topk(r.cand(), 0.5)[0, 0, 0].tolist() == [False, True, True, True, False, False]
    assert r.select_topk(r.cand(1, 1), 0.5)[0, 0, 0].tolist() == [False, True, True, False, False, False]
    assert r.map("topk", 0.5, 1, 1)[0, 0, 0].tolist() == [True, True, True, False, False, True]
    pk[0, 0, :, 0] = torch.tensor([-0.0, 0.0, -0.0, 0.0, -1.0, 0.0])  # +0 and -0 are one value: index order decides
    r = S.Rule(pq, ones[..., :1], pk, ones, 1.0, 0.5)
    assert r.select_topk(r.cand(), 0.5)[0, 0, 0].tolist() == [True, True, True, False, False, False]


@pytest.mark.parametrize("name", list(U.CASES))
def test_equal_length_consequence_and_forced_tiles(name):
    """Under TOPK every self-similar q-block of one (b, h_q) has exactly (ntk - n) + kcount active tiles."""
    r = S.rule_of_case(name)
    topk = torch.tensor(([0.3, 1.0, 0.125, 0.5] * 2)[:r.Hq])
    for kf, kl in S.KEEPS + ((0, 200), (1 << 30, 0)):
        cand = r.cand(kf, kl)
        n, kc = cand.sum(-1), r.kc(cand, topk)
        m = r.map("topk", topk, kf, kl)
        want = (r.ntk - n + kc).expand(-1, -1, r.nqb)
        ss = r.selfsim.squeeze(-1)
        assert torch.equal(m.sum(-1)[ss], want[ss])
        assert m[~ss].all() and m.any(-1).all()
        assert m[(~cand).expand_as(m)].all()                              # kept and ineligible tiles: on in every row
        assert ((m & cand).sum(-1)[ss] == kc.expand(-1, -1, r.nqb)[ss]).all()
        if kf + kl >= r.ntk:
            assert m.all()                                                # n == 0: every tile of the row is on
    full = r.map("topk", 1.0)
    assert full.all() and torch.equal(r.map("topk", float("nan")), full)


@pytest.mark.parametrize("name", list(U.CASES))
def test_cdf_without_keeps_is_todays_rule(name):
    ref = U.ref(name)
    r = S.Rule(ref.pq, ref.sq, ref.pk, ref.sk, ref.sm_scale, ref.simthr)  # the fp64 statistics of sparge_util.Ref
    for cdf in U.CDFS + (0.0, 1.0):
        assert torch.equal(r.map("cdf", cdf), ref.map(cdf)), cdf
    # kept blocks leave the softmax: the mass is taken over the candidates only
    cand = r.cand(2, 1)
    sel, p = r.select_cdf(cand, 0.9)
    live = r.live(cand)
    assert not (sel & ~cand).any() and ((p * cand).sum(-1)[live] - 1).abs().max() < 1e-12
    assert ((p * sel).sum(-1) >= 0.9 - 1e-12)[live].all()


# ---- 3. the condition on the inputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keeps", S.KEEPS)
@pytest.mark.parametrize("topk", S.TOPKS)
@pytest.mark.parametrize("name", list(U.CASES))
def test_input_condition_rows_are_firm(name, topk, keeps):
    """With float32 pooling in torch: at most 1/16 of the live rows of a combination may be not firm (a condition on the
    inputs, not a tolerance), and on these inputs a firm row is strictly firm -- no candidate outside the top set can reach
    any member of it within the bounds -- which is what lets the GPU test ask for the exact set on firm rows."""
    r = S.rule_of_case(name)
    cand = r.cand(*keeps)
    live = r.live(cand)
    firm, strict = r.firm(cand, topk)
    assert live.any() and int(live.sum()) >= 16
    kc, n = r.kc(cand, topk), cand.sum(-1)
    assert ((kc >= 1) & (kc < n)).all()  # a real cut in every head
    notfirm = int((live & ~firm).sum())
    print(f"{name} topk {topk} keeps {keeps}: live rows {int(live.sum())}, not firm {notfirm}")
    assert notfirm <= S.NONFIRM_CAP * int(live.sum()), (notfirm, int(live.sum()))
    assert not (firm & ~strict & live).any()
