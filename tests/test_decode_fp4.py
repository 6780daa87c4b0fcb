"""Decode attention on the paged MXFP4 V cache (include/sageattn_hip_decode_fp4.h) without a GPU: the new header against its
ctypes table, the refusals and the shapes of the fake ops.  What the kernel computes: test_decode_fp4_gpu.py."""
import ctypes

import pytest
import torch

from test_prefix import _cpu_whole, _prototypes

NS = "sageattention_amd_decode_fp4"


def test_header_matches_its_table():
    from sageattention_amd import _lib as L
    protos = _prototypes("sageattn_hip_decode_fp4.h")
    name = "sage_attn_fusedq_pv_f4_decode_paged"
    assert list(protos) == list(L.DECODE_FP4_SIGNATURES) == [name]
    (ret, params), (res, args) = protos[name], L.DECODE_FP4_SIGNATURES[name]
    want = {"int": ctypes.c_int, "sage_stream_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float}
    assert res is want[ret] and len(params) == len(args) == 29
    for c, ct in zip(params, args):
        assert ct is (ctypes.POINTER(L.SageTensor) if c == "sage_tensor*" else ctypes.c_void_p if c.endswith("*") else want[c])
    # the paged FP4 entry's prototype without `causal`, the argument behind num_splits
    paged = L.PAGED_FP4_SIGNATURES["sage_attn_fusedq_pv_f4_splitkv_paged"][1]
    assert args == paged[:-5] + paged[-4:]
    fn = getattr(L.lib(), name)
    assert fn.restype is res and fn.argtypes == args
    assert len(L.SIGNATURES) == 69 and L.lib().sage_abi_version() == 3        # the core header is what it was


def _v4(layout="HND"):
    """a SagePagedKVCacheV4 of 3 sequences with zero state on the CPU: Hk = 2, head_dim 64, pages of 128 keys"""
    import sageattention_amd as sa
    return sa.SagePagedKVCacheV4(_cpu_whole(layout=layout), torch.zeros(8, 2, 64, 64, dtype=torch.uint8),
                                 torch.full((8, 2, 2, 128), 127, dtype=torch.uint8))


def test_refusals():
    """raised before any device call (the tensors are on the CPU), in the words of sageattn_splitkv_paged_v4(causal=True)"""
    import sageattention_amd as sa
    assert {"sageattn_decode_paged_v4", "sageattn_decode_paged_v4_compilable"} <= set(sa.__all__)
    cache = _v4()
    table, lens = torch.zeros(3, 3, dtype=torch.int32), torch.tensor([80, 3, 0], dtype=torch.int32)
    q = torch.zeros(3, 2, 8, 64, dtype=torch.float16)
    f = lambda qq=q, c=cache, **kw: sa.sageattn_decode_paged_v4(qq, c, table, lens, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="at most 32 query rows.*sageattn_splitkv_paged_v4"):
        f(torch.zeros(3, 2, 36, 64, dtype=torch.float16), q_fold=4)
    with pytest.raises(TypeError, match="SagePagedKVCacheV4"):
        f(c=_cpu_whole())
    for kw, exc in (({"q_fold": 3}, ValueError), ({"q_fold": 2.0}, TypeError), ({"num_splits": 17}, ValueError),
                    ({"window": 3}, TypeError), ({"qq": q.to(torch.bfloat16)}, ValueError), ({"qq": q[..., :32]}, ValueError)):
        with pytest.raises(exc) as mine:
            f(**kw)
        with pytest.raises(exc) as parents:
            sa.sageattn_splitkv_paged_v4(kw.pop("qq", q), cache, table, lens, causal=True, **kw)
        assert str(mine.value) == str(parents.value)


def test_op_names_and_fake_shapes():
    ops = getattr(torch.ops, NS)
    assert sorted(n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith(NS + "::")) == \
        ["attn_decode_paged_v4", "attn_decode_paged_v4_lse"]
    for layout, shape in (("HND", (3, 2, 12, 64)), ("NHD", (3, 12, 2, 64))):
        c = _v4(layout)
        q = torch.empty(shape, dtype=torch.float16, device="meta")
        args = [t.to("meta") for t in (c.k8, c.k_scale, c.km, c.v4, c.v4_scale)] + [
            torch.empty(3, 3, dtype=torch.int32, device="meta"), torch.empty(3, dtype=torch.int32, device="meta")]
        o, lse = ops.attn_decode_paged_v4_lse(q, *args, 0, 4, layout, 0.125, "per_thread")
        assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == (3, 2, 12) and lse.dtype == torch.float32
        assert ops.attn_decode_paged_v4(q, *args, 3, 4, layout, 0.125, "per_thread").shape == q.shape
