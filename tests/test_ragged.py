"""Ragged-query attention on the paged cache (``sageattn_splitkv_paged_ragged``, include/sageattn_hip_ragged.h) without a GPU:
the new header against its ctypes table, the Python refusals and the schemas of the ops.  What the
kernels compute: test_ragged_gpu.py."""
import ctypes

import pytest
import torch

from test_prefix import _cpu_whole, _prototypes

NS = "sageattention_amd_ragged"
ENTRIES = {"sage_ragged_q_plan": 7, "sage_ragged_workspace_bytes": 4, "sage_attn_fusedq_pv_f16_splitkv_paged_ragged": 32,
           "sage_attn_fusedq_pv_f8_splitkv_paged_ragged": 32}


def test_header_matches_its_table():
    from sageattention_amd import _lib as L
    protos = _prototypes("sageattn_hip_ragged.h")
    assert {n: len(p) for n, (_, p) in protos.items()} == {n: len(a) for n, (_, a) in L.RAGGED_SIGNATURES.items()} == ENTRIES
    want = {"int": ctypes.c_int, "sage_stream_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float}
    for name, (ret, params) in protos.items():
        res, args = L.RAGGED_SIGNATURES[name]
        assert res is want[ret], name
        for c, ct in zip(params, args):
            if c == "sage_tensor*":
                assert ct is ctypes.POINTER(L.SageTensor), (name, c)
            else:
                assert ct is (ctypes.c_void_p if c.endswith("*") else want[c]), (name, c)
        fn = getattr(L.lib(), name)
        assert fn.restype is res and fn.argtypes == args
    assert len(L.SIGNATURES) == 69 and L.lib().sage_abi_version() == 3        # the core header is what it was


def test_refusals():
    """raised before any device call (the tensors are on the CPU)"""
    import sageattention_amd as sa
    assert {"RaggedQPlan", "ragged_q_plan", "sageattn_splitkv_paged_ragged"} <= set(sa.__all__)
    f = sa.sageattn_splitkv_paged_ragged
    cache = _cpu_whole()                                                          # 3 sequences, Hk = 2, head_dim 64
    q = torch.zeros(9, 4, 64, dtype=torch.float16)
    table, lens = torch.zeros(3, 3, dtype=torch.int32), torch.tensor([80, 3, 0], dtype=torch.int32)
    cu = torch.tensor([0, 1, 6, 9], dtype=torch.int32)
    for bad in (0, 3, 4, -1):                                                     # q_fold: 1 or Hq / Hk = 2
        with pytest.raises(ValueError, match="q_fold"):
            f(q, cache, table, lens, cu, q_fold=bad)
    with pytest.raises(TypeError, match="q_fold"):
        f(q, cache, table, lens, cu, q_fold=2.0)
    v4 = sa.SagePagedKVCacheV4(cache, None, None)
    with pytest.raises(TypeError, match="SagePagedKVCacheV4.*not built"):
        f(q, v4, table, lens, cu)
    with pytest.raises(TypeError, match="SagePagedKVCache or a SagePagedRowCache"):
        f(q, object(), table, lens, cu)
    # the keywords sageattn_splitkv_paged refuses, in its words; `causal` is no keyword here
    for kw in (dict(attn_mask=torch.zeros(1)), dict(is_causal=False), dict(smooth_k=False), dict(cu_seqlens_k=cu)):
        with pytest.raises(ValueError, match="sageattn_splitkv_causal does not take") as mine:
            f(q, cache, table, lens, cu, **kw)
        with pytest.raises(ValueError) as theirs:
            sa.sageattn_splitkv_paged(torch.zeros(3, 4, 8, 64, dtype=torch.float16), cache, table, lens, causal=True, **kw)
        assert str(mine.value) == str(theirs.value)
    for kw in (dict(causal=True), dict(tensor_layout="HND")):
        with pytest.raises(TypeError, match="unexpected keyword"):
            f(q, cache, table, lens, cu, **kw)
    with pytest.raises(TypeError, match="cu_seqlens_q must be an int32 tensor"):
        f(q, cache, table, lens, [0, 1, 6, 9])
    with pytest.raises(TypeError, match="cu_seqlens_q must be of dtype int32"):
        f(q, cache, table, lens, cu.long())
    for bad in (cu.view(1, 4), cu[:1], torch.zeros((), dtype=torch.int32)):
        with pytest.raises(ValueError, match="cu_seqlens_q shape"):
            f(q, cache, table, lens, bad)
    with pytest.raises(ValueError, match="block_table shape"):                    # B comes from cu_seqlens_q
        f(q, cache, table, lens, cu[:3])
    with pytest.raises(ValueError, match="kv_lens shape"):
        f(q, cache, table, lens[:2], cu)
    with pytest.raises(TypeError, match="kv_lens"):
        f(q, cache, table, None, cu)
    for bad in (q.unsqueeze(0), q[:0], q.transpose(1, 2)):
        with pytest.raises(ValueError, match="q must"):
            f(bad, cache, table, lens, cu)
    with pytest.raises(ValueError, match="head_dim"):
        f(torch.zeros(9, 4, 128, dtype=torch.float16), cache, table, lens, cu)
    with pytest.raises(ValueError, match="divisible"):
        f(torch.zeros(9, 3, 64, dtype=torch.float16), cache, table, lens, cu)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="num_splits"):
            f(q, cache, table, lens, cu, num_splits=bad)
    with pytest.raises(TypeError, match="plan must be a RaggedQPlan"):
        f(q, cache, table, lens, cu, plan=torch.zeros(4, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="plan was made for"):
        f(q, cache, table, lens, cu, plan=sa.RaggedQPlan(torch.zeros(3, 2, dtype=torch.int32), 3, 9, 1), q_fold=2)
    with pytest.raises(ValueError, match="total_tokens"):
        sa.ragged_q_plan(cu, 0)
    with pytest.raises(TypeError, match="cu_seqlens_q must be of dtype int32"):
        sa.ragged_q_plan(cu.float(), 9)


def test_op_schemas():
    import sageattention_amd  # noqa: F401
    names = torch._C._dispatch_get_all_op_names()
    ops = ("ragged_q_plan", "attn_splitkv_paged_ragged", "attn_splitkv_paged_ragged_lse")
    assert sorted(n.split("::")[1] for n in names if n.startswith(NS + "::")) == sorted(ops)
    schema = lambda n: str(getattr(getattr(torch.ops, NS), n).default._schema)  # noqa: E731
    assert schema("ragged_q_plan") == f"{NS}::ragged_q_plan(Tensor cu_seqlens_q, SymInt total_tokens, SymInt q_fold) -> Tensor"
    params = ("(Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor block_table, Tensor kv_lens, "
              "Tensor cu_seqlens_q, Tensor items, SymInt num_splits, SymInt q_fold, str tensor_layout, float sm_scale, "
              "str qk_quant_gran)")
    assert schema("attn_splitkv_paged_ragged") == f"{NS}::attn_splitkv_paged_ragged{params} -> Tensor"
    assert schema("attn_splitkv_paged_ragged_lse") == f"{NS}::attn_splitkv_paged_ragged_lse{params} -> (Tensor, Tensor)"
