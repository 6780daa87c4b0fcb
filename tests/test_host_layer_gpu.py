"""The Python host layer in front of the attention kernels (core._prepass, core._block_sparse_tail, core._pack), on the GPU:
``sageattn_sparge`` is ``sageattn_block_sparse`` on its own plan, every combination of the return flags gives the documented
pieces in the documented order, and the three branches of the K / V pre-pass feed the same kernel bits.

q (1, 2, 200, D) and k / v (1, 1, 333, D): one full and one ragged 128-row q-block; six key tiles, the last ragged -- more
than the four-slot ring plus its read-ahead of five list entries, so prologue, steady state, tail and list padding all run,
with two query heads on one key head.

Asserted elsewhere and not repeated: the three-way equality of (a) on the firm inputs of tests/pvskip_util.py, with HIP-graph
capture and torch.compile (test_pvskip_gpu.py::test_operator_capture_and_compile); one call against the multi-call path
(test_one_call.py); fused against stand-alone Q quantizer on the golden shapes (test_gpu_parity.py)."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, THR = 200, 333, 3.0
CASES = [(D, pv) for D in (64, 128) for pv in ("fp16", "fp8")]


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    import sageattention_amd.ops  # noqa: F401  (registers the ops)
    return sageattention_amd


@pytest.fixture(scope="module")
def inputs():
    """Per head_dim: q with logits of a few units, and keys 128 .. 255 (tiles 2 and 3) set to the mean key, so that their
    smoothed scores are near 0, far below the running maximum of every row: the waves skip them (pvthreshd = THR).  Random
    query rows are not alike, so the predictor keeps every tile of every q-block."""
    out = {}
    for D in (64, 128):
        g = torch.Generator().manual_seed(D)
        q = (torch.randn(1, 2, M, D, generator=g) * 4).half()
        k = torch.randn(1, 1, N, D, generator=g)
        k[:, :, 128:256] = k.mean(dim=2, keepdim=True)
        v = torch.randn(1, 1, N, D, generator=g).half()
        out[D] = tuple(t.cuda() for t in (q, k.half(), v))
    return out


@pytest.fixture(scope="module")
def all_on(sa, inputs):
    """(D, pv) -> (o, lse, plan, skipped) of sageattn_sparge with every return flag on: computed once, left unchanged"""
    out = {}
    for D, pv in CASES:
        out[D, pv] = sa.sageattn_sparge(*inputs[D], pv=pv, return_lse=True, return_plan=True, pvthreshd=THR,
                                        return_skipped=True)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("D,pv", CASES)
def test_sparge_is_block_sparse_on_its_plan(sa, inputs, all_on, D, pv):
    """(a) sageattn_sparge, sageattn_block_sparse on the plan it returned, and sageattn_sparge_compilable: o, lse and the skip
    counters bit-equal"""
    from sageattention_amd.ops import sageattn_sparge_compilable
    q, k, v = inputs[D]
    o, lse, plan, sk = all_on[D, pv]
    assert o.shape == q.shape and lse.shape == (1, 2, M) and sk.shape == (1, 2, 2, 4) and sk.dtype == torch.int32
    assert (plan.B, plan.Hq, plan.M, plan.N) == (1, 2, M, N)
    assert int(plan.lists.view(1, 2, 2, -1)[..., 0].min()) == 6, "the predictor was meant to keep all six tiles"
    assert int(sk.sum()) > 0, "the inputs were meant to make waves skip tiles"
    o2, lse2, sk2 = sa.sageattn_block_sparse(q, k, v, plan, pv=pv, return_lse=True, pvthreshd=THR, return_skipped=True)
    o3, lse3, sk3 = sageattn_sparge_compilable(q, k, v, pv=pv, return_lse=True, pvthreshd=THR, return_skipped=True)
    torch.cuda.synchronize()
    for name, a, b, c in (("o", o, o2, o3), ("lse", lse, lse2, lse3), ("skipped", sk, sk2, sk3)):
        assert torch.equal(a, b), f"{name}: sageattn_block_sparse on the returned plan differs"
        assert torch.equal(a, c), f"{name}: sageattn_sparge_compilable differs"


@pytest.mark.parametrize("D,pv", CASES)
def test_return_flags(sa, inputs, all_on, D, pv):
    """(b) the eight combinations of return_lse / return_plan / return_skipped: o, then lse, plan and skipped, each when asked
    for, a bare tensor when only o is; every piece bit-equal to the call with all three on"""
    q, k, v = inputs[D]
    o, lse, plan, sk = all_on[D, pv]
    for want_lse, want_plan, want_sk in itertools.product((False, True), repeat=3):
        got = sa.sageattn_sparge(q, k, v, pv=pv, return_lse=want_lse, return_plan=want_plan, pvthreshd=THR,
                                 return_skipped=want_sk)
        torch.cuda.synchronize()
        flags = (want_lse, want_plan, want_sk)
        if not any(flags):
            assert isinstance(got, torch.Tensor) and torch.equal(got, o), flags
            continue
        assert isinstance(got, tuple) and len(got) == 1 + sum(flags), flags
        rest = list(got[1:])
        assert torch.equal(got[0], o), flags
        if want_lse:
            assert torch.equal(rest.pop(0), lse), flags
        if want_plan:
            p = rest.pop(0)
            assert isinstance(p, sa.BlockSparsePlan) and (p.B, p.Hq, p.M, p.N) == (1, 2, M, N), flags
            assert torch.equal(p.lists, plan.lists), flags
        if want_sk:
            assert torch.equal(rest.pop(0), sk), flags
        assert rest == []


@pytest.mark.parametrize("form", [dict(smooth_k=False), dict(smooth_v=True, pv_accum_dtype="fp32")],
                         ids=["no_smooth_k", "smooth_v"])
@pytest.mark.parametrize("D", [64, 128])
def test_fp8_multi_call_prepass_branches(sa, inputs, D, form):
    """(c) sageattn_qk_int8_pv_fp8_cuda on the multi-call path (ONE_CALL off) where K and V are NOT prepared by one call: K
    without smoothing, and V with its mean taken out (honoured with pv_accum_dtype "fp32").  The identity the suite uses
    for this path (test_gpu_parity.py::test_fused_q_quantizer_is_bit_identical): the Q quantizer folded into the kernel and
    the stand-alone one give the same o bit for bit, and the LSE to 1e-5 (the q.km dot is summed in another order)."""
    from sageattention_amd import core
    q, k, v = inputs[D]
    keep = core.ONE_CALL, core.FUSE_Q_QUANT
    try:
        core.ONE_CALL = False
        core.FUSE_Q_QUANT = True
        o1, l1 = sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, return_lse=True, **form)
        o1_only = sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, **form)
        core.FUSE_Q_QUANT = False
        o0, l0 = sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, return_lse=True, **form)
    finally:
        core.ONE_CALL, core.FUSE_Q_QUANT = keep
    torch.cuda.synchronize()
    assert torch.equal(o1, o0), (o1.float() - o0.float()).abs().max()
    assert torch.equal(o1, o1_only)
    assert (l1 - l0).abs().max() < 1e-5 * max(1.0, float(l0.abs().max()))
    assert torch.isfinite(o1.float()).all() and torch.isfinite(l1).all()
