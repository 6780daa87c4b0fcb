"""Decode attention on the paged cache (include/sageattn_hip_decode.h) without a GPU: the new header against its ctypes table,
the refusals, the split rule and the shapes of the fake ops.  What the kernel computes: test_decode_gpu.py."""
import ctypes

import pytest
import torch

from test_prefix import _cpu_whole, _prototypes

NS = "sageattention_amd_decode"


def test_header_matches_its_table():
    from sageattention_amd import _lib as L
    protos = _prototypes("sageattn_hip_decode.h")
    names = {f"sage_attn_fusedq_pv_{pv}_decode_paged": 29 for pv in ("f16", "f8")}
    assert {n: len(p) for n, (_, p) in protos.items()} == {n: len(a) for n, (_, a) in L.DECODE_SIGNATURES.items()} == names
    want = {"int": ctypes.c_int, "sage_stream_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float}
    for name, (ret, params) in protos.items():
        res, args = L.DECODE_SIGNATURES[name]
        assert res is want[ret], name
        for c, ct in zip(params, args):
            assert ct is (ctypes.POINTER(L.SageTensor) if c == "sage_tensor*" else ctypes.c_void_p if c.endswith("*") else want[c])
        # the paged entry's prototype without `causal`, the argument behind num_splits
        paged = L.PAGED_SIGNATURES[name.replace("_decode_paged", "_splitkv_paged")][1]
        assert args == paged[:-5] + paged[-4:]
        fn = getattr(L.lib(), name)
        assert fn.restype is res and fn.argtypes == args
    assert len(L.SIGNATURES) == 69 and L.lib().sage_abi_version() == 3        # the core header is what it was


@pytest.mark.parametrize("rows", [False, True])
def test_refusals(rows):
    """raised before any device call (the tensors are on the CPU), in the words of sageattn_splitkv_paged where it has them"""
    import sageattention_amd as sa
    assert {"sageattn_decode_paged", "sageattn_decode_paged_compilable", "decode_num_splits"} <= set(sa.__all__)
    cache = _cpu_whole(rows=rows)                                                 # 3 sequences, Hk = 2, head_dim 64
    table, lens = torch.zeros(3, 3, dtype=torch.int32), torch.tensor([80, 3, 0], dtype=torch.int32)
    q = torch.zeros(3, 2, 8, 64, dtype=torch.float16)
    f = lambda qq=q, c=cache, **kw: sa.sageattn_decode_paged(qq, c, table, lens, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="at most 32 query rows.*sageattn_splitkv_paged"):
        f(torch.zeros(3, 2, 36, 64, dtype=torch.float16), q_fold=4)
    for kw, exc in (({"q_fold": 3}, ValueError), ({"q_fold": 2.0}, TypeError), ({"num_splits": 17}, ValueError),
                    ({"is_causal": False}, ValueError), ({"window": 3}, TypeError), ({"c": object()}, TypeError),
                    ({"c": sa.SagePagedKVCacheV4(cache, None, None)}, TypeError),
                    ({"qq": q.to(torch.bfloat16)}, ValueError), ({"qq": q[..., :32]}, ValueError)):
        with pytest.raises(exc) as mine:
            f(**kw)
        kw.setdefault("c", cache)
        with pytest.raises(exc) as parents:
            sa.sageattn_splitkv_paged(kw.pop("qq", q), kw.pop("c"), table, lens, causal=True, **kw)
        assert str(mine.value) == str(parents.value)


def test_num_splits_and_fake_shapes():
    import sageattention_amd as sa
    assert [sa.decode_num_splits(*a) for a in ((8, 8, 8192), (64, 8, 8192), (1, 8, 65536), (1, 1, 100), (1, 1, 0))] == [12, 1, 16, 1, 1]
    assert sa.decode_num_splits(8, 16, 8192) == 6 and sa.decode_num_splits(2, 1, 512) == 2
    assert sa.decode_num_splits(8, 9, 8192) == 10                          # 768 / 72 rounded DOWN: the grid fits the resident slots
    ops = getattr(torch.ops, NS)
    assert sorted(n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith(NS + "::")) == \
        ["attn_decode_paged", "attn_decode_paged_lse"]
    for layout, shape in (("HND", (3, 2, 12, 64)), ("NHD", (3, 12, 2, 64))):
        c = _cpu_whole(layout=layout)
        q = torch.empty(shape, dtype=torch.float16, device="meta")
        args = [t.to("meta") for t in (c.k8, c.k_scale, c.km, c.v)] + [None, torch.empty(3, 3, dtype=torch.int32, device="meta"),
                                                                        torch.empty(3, dtype=torch.int32, device="meta")]
        o, lse = ops.attn_decode_paged_lse(q, *args, 0, 4, layout, 0.125, "per_thread")
        assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == (3, 2, 12) and lse.dtype == torch.float32
        assert ops.attn_decode_paged(q, *args, 3, 4, layout, 0.125, "per_thread").shape == q.shape
