"""The block-map predictor without a GPU: its C-ABI entry points check every argument before their first launch, the torch
restatement of the rule (tests/sparge_util.py) is sound, and the clustered test inputs meet the conditions under which the
GPU tests (tests/test_sparge_gpu.py) may compare an fp32 kernel with an fp64 reference."""
import pytest
import torch

import sparge_util as U

# ---- 1. every argument is checked before the first launch -------------------------------------------------------------
# Fake device addresses: where a GPU is visible a missed check would launch kernels on them, so this runs only where none
# is; there every launch attempt returns SAGE_ERR_LAUNCH (-5), which makes a launch observable (tests/test_block_sparse.py).
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")

FAKE = 1 << 20
ODD = FAKE + 8

_PARAMS = {
    "sage_block_pool_sim": "x dtype B H N D blk mean pooled sim stream",
    "sage_block_select_cdf": "pq sq pk sk B Hq Hk M N D sm thr cdf lists nbytes map stream",
}


def _valid(fn):
    from sageattention_amd import _lib as L
    if fn == "sage_block_pool_sim":
        return dict(x=L.SageTensor(FAKE, 1 << 16, 1 << 12, 64), dtype=0, B=1, H=2, N=333, D=64, blk=64, mean=FAKE, pooled=FAKE,
                    sim=FAKE, stream=None)
    B, Hq, M, N = 1, 2, 200, 333
    return dict(pq=FAKE, sq=FAKE, pk=FAKE, sk=FAKE, B=B, Hq=Hq, Hk=1, M=M, N=N, D=64, sm=0.125, thr=FAKE, cdf=FAKE, lists=FAKE,
                nbytes=L.lib().sage_block_sparse_workspace_bytes(B, Hq, M, N), map=None, stream=None)


def _call(fn, **change):
    from sageattention_amd import _lib as L
    args = dict(_valid(fn), **change)
    return getattr(L.lib(), fn)(*[args[n] for n in _PARAMS[fn].split()])


@no_gpu
def test_valid_calls_reach_a_launch():
    assert [fn for fn in _PARAMS if _call(fn) != -5] == []
    assert _call("sage_block_pool_sim", mean=None, blk=128, D=128, dtype=1) == -5
    assert _call("sage_block_select_cdf", map=FAKE + 1) == -5  # the map is bytes: no alignment asked
    assert _call("sage_block_select_cdf", N=2048 * 64, nbytes=1 << 40) == -5  # the largest N the LDS row holds


@no_gpu
def test_single_fault_status_table():
    """Each argument made invalid on its own returns its argument status: nothing was launched (a launch returns -5 here)."""
    from sageattention_amd import _lib as L
    t = lambda data=FAKE, sn=64: L.SageTensor(data, 1 << 16, 1 << 12, sn)  # noqa: E731
    pool, sel = "sage_block_pool_sim", "sage_block_select_cdf"
    need = _valid(sel)["nbytes"]
    cases = [(pool, c, -1) for c in (
        dict(x=None), dict(x=t(0)), dict(x=t(ODD)), dict(x=t(sn=4)), dict(pooled=None), dict(pooled=ODD), dict(sim=None),
        dict(mean=ODD), dict(dtype=7), dict(blk=32), dict(blk=0), dict(blk=256), dict(B=0), dict(H=0), dict(N=0), dict(N=-5))]
    cases += [(pool, dict(D=96), -2), (pool, dict(D=0), -2)]
    cases += [(sel, c, -1) for c in (
        dict(pq=None), dict(pq=ODD), dict(sq=None), dict(pk=None), dict(pk=ODD), dict(sk=None), dict(thr=None), dict(cdf=None),
        dict(lists=None), dict(lists=ODD), dict(nbytes=need - 4), dict(nbytes=0), dict(B=0), dict(Hq=0), dict(Hk=0),
        dict(Hq=3, Hk=2), dict(M=0), dict(N=0), dict(sm=0.0), dict(sm=-1.0), dict(sm=float("nan")), dict(sm=float("inf")),
        # a list buffer sized for fewer keys than the call has
        dict(nbytes=L.lib().sage_block_sparse_workspace_bytes(1, 2, 200, 64)))]
    cases += [(sel, dict(D=96), -2), (sel, dict(N=2048 * 64 + 1, nbytes=1 << 40), -4), (sel, dict(N=1 << 25, nbytes=1 << 40), -4)]
    wrong = [(fn, sorted(c), st, got) for fn, c, st in cases if (got := _call(fn, **c)) != st]
    assert not wrong, wrong


def test_python_errors_and_exports():
    import sageattention_amd as sa
    import sageattention_amd.ops as ops
    assert {"sageattn_sparge", "sparge_plan"} <= set(sa.__all__) and "sageattn_sparge_compilable" in ops.__all__
    q = torch.zeros(1, 2, 300, 64, dtype=torch.float16)
    with pytest.raises(AssertionError, match="cuda"):
        sa.sparge_plan(q, q)
    with pytest.raises(AssertionError, match="cuda"):
        sa.sageattn_sparge(q, q, q)
    with pytest.raises(ValueError, match="pv"):
        sa.sageattn_sparge(q, q, q, pv="auto")
    with pytest.raises(ValueError, match="qk_quant_gran"):
        sa.sageattn_sparge(q, q, q, qk_quant_gran="per_block")
    with pytest.raises(TypeError):  # non-causal only: there is no is_causal to pass
        sa.sageattn_sparge(q, q, q, is_causal=True)
    with pytest.raises(ValueError):
        ops.sageattn_sparge_compilable(q, q, q, tensor_layout="BHSD")


def test_op_schema_and_fake_shapes():
    import sageattention_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    s = str(torch.ops.sageattention_amd.attn_sparge.default._schema)
    assert ("Tensor q, Tensor k, Tensor v, Tensor simthreshd1, Tensor cdfthreshd, str tensor_layout, float sm_scale, str pv, "
            "str qk_quant_gran") in s
    assert str(torch.ops.sageattention_amd.attn_sparge_lse.default._schema).endswith("-> (Tensor, Tensor)")
    with FakeTensorMode():
        for layout, shp, kshp in (("HND", (2, 8, 300, 96), (2, 4, 333, 96)), ("NHD", (2, 300, 8, 96), (2, 333, 4, 96))):
            q = torch.empty(shp, dtype=torch.bfloat16, device="cuda")
            k = torch.empty(kshp, dtype=torch.bfloat16, device="cuda")
            o, lse = ops.sageattn_sparge_compilable(q, k, k, tensor_layout=layout, pv="fp8", cdfthreshd=0.9, return_lse=True)
            assert o.shape == q.shape and o.dtype == q.dtype and o.device == q.device and o.is_contiguous()
            assert lse.shape == (2, 8, 300) and lse.dtype == torch.float32


# ---- 2. the restatement checks itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "c3"])
def test_sim_is_the_mean_of_the_cosine_matrix(name):
    """|sum of unit rows|^2 / c^2 is the mean of the c x c cosine matrix, ragged last blocks (50 rows, 37 rows, 1 row)
    included; with and without a mean."""
    r = U.ref(name)
    for x, blk, mean in ((r.q, 128, None), (r.k, 64, r.km), (r.k, 64, None)):
        _, sim = U.pool_sim(x, blk, mean)
        assert (sim - U.sim_explicit(x, blk, mean)).abs().max() < 1e-12
    z = torch.zeros(1, 1, 70, 64, dtype=torch.float16)  # rows of zero norm contribute the zero vector
    z[0, 0, 0, 0] = 1.0
    pooled, sim = U.pool_sim(z, 64)
    assert torch.equal(sim, torch.tensor([[[1.0 / 64 ** 2, 0.0]]], dtype=torch.float64)) and pooled[0, 0, 0, 0] == 1.0 / 64


@pytest.mark.parametrize("name", list(U.CASES))
def test_selection_is_monotone_and_complete_at_one(name):
    r = U.ref(name)
    prev = None
    for cdf in (0.0, 0.3, 0.5, 0.9, 0.98, 0.999):
        sel = U.select(r.p, r.elig, cdf)
        assert not (sel & ~r.elig).any()
        assert (sel.any(-1) == r.elig.any(-1).expand_as(sel.any(-1))).all()  # never empty when an eligible block exists
        assert prev is None or not (prev & ~sel).any()                       # monotone in cdfthreshd
        prev = sel
        assert U.full_map(sel, r.elig, r.selfsim).any(-1).all()              # every list has at least one tile
    for cdf in (1.0, 1.5):
        assert torch.equal(U.select(r.p, r.elig, cdf), r.elig.expand_as(r.p))
        assert r.map(cdf).all()                                              # cdfthreshd = 1 turns every tile on
    assert (U.select(r.p, r.elig, 0.0).sum(-1) == r.elig.any(-1)).all()      # the top block alone
    # per-head thresholds are the per-head selections
    cdf = torch.tensor([1.0] + [0.5] * (r.Hq - 1))
    mixed = U.select(r.p, r.elig, cdf)
    assert torch.equal(mixed[:, 0], r.elig.expand_as(r.p)[:, 0]) and torch.equal(mixed[:, 1:], U.select(r.p, r.elig, 0.5)[:, 1:])


def test_ties_go_to_the_lower_index():
    p = torch.tensor([0.1, 0.2, 0.2, 0.2, 0.2, 0.1], dtype=torch.float64).view(1, 1, 1, 6)
    elig = torch.ones(1, 1, 1, 6, dtype=torch.bool)
    assert U.select(p, elig, 0.5)[0, 0, 0].tolist() == [False, True, True, True, False, False]


# ---- 3. the conditions on the inputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.CASES))
def test_input_conditions(name):
    """What lets the GPU tests compare an fp32 kernel with the fp64 rule exactly, checked on the inputs themselves:
    no eligibility decision near its threshold, few rows whose selection flips within cdfthreshd +- DELTA, no near-tie at the
    cut of the other rows, and a score error well inside DELTA."""
    r = U.ref(name)
    assert r.gap[1] - r.gap[0] >= 0.1, r.gap
    # the smoothing mean matters on these inputs: without it every K block looks self-similar
    assert U.pool_sim(r.k, 64, None)[1].min() > 0.85 and r.sk.min() < 0.3
    assert (~r.elig).any() and r.elig.any() and r.live.any()
    assert bool((~r.selfsim).any()) == (r.M > 3 * 128)  # every 4th q-block is noise
    rows = r.selfsim.numel()
    for cdf in (0.5, 0.9):
        marg = r.marginal(cdf)
        assert int(marg.sum()) <= 0.25 * rows, (cdf, int(marg.sum()), rows)
        sel = U.select(r.p, r.elig, cdf)
        last_in = torch.where(sel, r.p, torch.full_like(r.p, float("inf"))).amin(-1)
        first_out = torch.where(r.elig & ~sel, r.p, torch.zeros_like(r.p)).amax(-1)
        near_tie = (first_out >= last_in * (1 - 1e-4)) & r.live & ~marg
        assert not near_tie.any(), (cdf, int(near_tie.sum()))
    # fp32 score error of any summation order, (D + 2) roundings on each side, and the softmax's own (ntk + 8)
    g = r.Hq // r.Hk
    s_abs = (r.pq.abs() @ r.pk.repeat_interleave(g, 1).abs().transpose(-1, -2)) * r.sm_scale
    bound = 2 * (r.D + 2) * 2.0 ** -24 * float(s_abs.max()) + (r.pk.shape[2] + 8) * 2.0 ** -24
    assert bound <= U.DELTA / 4, bound
