"""Sliding-window attention and sink logits on the paged cache (include/sageattn_hip_window.h) without a GPU: the new header
against its ctypes table, the refusals the window operators add to their parents', and the schemas of the ops.  What the
kernels compute: test_window_gpu.py."""
import ctypes

import pytest
import torch

from test_prefix import _cpu_whole, _prototypes

NS = "sageattention_amd_window"


def test_header_matches_its_table():
    from sageattention_amd import _lib as L
    protos = _prototypes("sageattn_hip_window.h")
    names = {f"sage_attn_fusedq_pv_{pv}_splitkv_paged_{r}window": n for pv in ("f16", "f8") for r, n in (("", 32), ("ragged_", 34))}
    assert {n: len(p) for n, (_, p) in protos.items()} == {n: len(a) for n, (_, a) in L.WINDOW_SIGNATURES.items()} == names
    want = {"int": ctypes.c_int, "sage_stream_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float}
    for name, (ret, params) in protos.items():
        res, args = L.WINDOW_SIGNATURES[name]
        assert res is want[ret], name
        for c, ct in zip(params, args):
            if c == "sage_tensor*":
                assert ct is ctypes.POINTER(L.SageTensor), (name, c)
            else:
                assert ct is (ctypes.c_void_p if c.endswith("*") else want[c]), (name, c)
        fn = getattr(L.lib(), name)
        assert fn.restype is res and fn.argtypes == args
    assert len(L.SIGNATURES) == 69 and L.lib().sage_abi_version() == 3        # the core header is what it was


@pytest.mark.parametrize("ragged", [False, True])
def test_refusals(ragged):
    """raised before any device call (the tensors are on the CPU)"""
    import sageattention_amd as sa
    assert {"sageattn_splitkv_paged_window", "sageattn_splitkv_paged_ragged_window"} <= set(sa.__all__)
    cache = _cpu_whole()                                                          # 3 sequences, Hk = 2, head_dim 64
    table, lens = torch.zeros(3, 3, dtype=torch.int32), torch.tensor([80, 3, 0], dtype=torch.int32)
    if ragged:
        q, cu = torch.zeros(9, 4, 64, dtype=torch.float16), torch.tensor([0, 1, 6, 9], dtype=torch.int32)
        f = lambda window, **kw: sa.sageattn_splitkv_paged_ragged_window(q, kw.pop("cache", cache), table, lens, cu, window, **kw)  # noqa: E731
    else:
        q = torch.zeros(3, 4, 8, 64, dtype=torch.float16)
        f = lambda window, **kw: sa.sageattn_splitkv_paged_window(q, kw.pop("cache", cache), table, lens, window, **kw)  # noqa: E731
    for bad in (0, -3):
        with pytest.raises(ValueError, match="window must be >= 1"):
            f(bad)
    for bad in (2.0, True, None):
        with pytest.raises(TypeError, match="window must be an int"):
            f(bad)
    for bad in (torch.zeros(3), torch.zeros(1, 4)):
        with pytest.raises(ValueError, match="sinks shape"):
            f(7, sinks=bad)
    with pytest.raises(TypeError, match="sinks must be of dtype float32"):
        f(7, sinks=torch.zeros(4, dtype=torch.float16))
    with pytest.raises(ValueError, match="sinks is on"):
        f(7, sinks=torch.zeros(4, device="meta"))
    with pytest.raises(TypeError, match="SagePagedKVCacheV4.*not built"):
        f(7, cache=sa.SagePagedKVCacheV4(cache, None, None))


def test_op_schemas():
    import sageattention_amd  # noqa: F401
    names = torch._C._dispatch_get_all_op_names()
    ops = [f"attn_splitkv_paged_{r}window{l}" for r in ("", "ragged_") for l in ("", "_lse")]
    assert sorted(n.split("::")[1] for n in names if n.startswith(NS + "::")) == sorted(ops)
    head = "(Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor block_table, Tensor kv_lens, "
    tail = "SymInt num_splits, SymInt q_fold, SymInt window, Tensor? sinks, str tensor_layout, float sm_scale, str qk_quant_gran)"
    for name in ops:
        mid = "Tensor cu_seqlens_q, Tensor items, " if "ragged" in name else ""
        ret = "(Tensor, Tensor)" if name.endswith("_lse") else "Tensor"
        assert str(getattr(getattr(torch.ops, NS), name).default._schema) == f"{NS}::{name}{head}{mid}{tail} -> {ret}"
