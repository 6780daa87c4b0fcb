"""Windowed decode attention with sink logits (include/sageattn_hip_decode_window.h) without a GPU: the new header against its
ctypes table, the refusals and the ops.  What the kernel computes: test_decode_window_gpu.py."""
import ctypes

import pytest
import torch

from test_prefix import _cpu_whole, _prototypes

NS = "sageattention_amd_decode_window"


def test_header_matches_its_table():
    from sageattention_amd import _lib as L
    protos = _prototypes("sageattn_hip_decode_window.h")
    names = {f"sage_attn_fusedq_pv_{pv}_decode_paged_window": 31 for pv in ("f16", "f8")}
    assert {n: len(p) for n, (_, p) in protos.items()} == {n: len(a) for n, (_, a) in L.DECODE_WINDOW_SIGNATURES.items()} == names
    want = {"int": ctypes.c_int, "sage_stream_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float}
    for name, (ret, params) in protos.items():
        res, args = L.DECODE_WINDOW_SIGNATURES[name]
        assert res is want[ret], name
        for c, ct in zip(params, args):
            assert ct is (ctypes.POINTER(L.SageTensor) if c == "sage_tensor*" else ctypes.c_void_p if c.endswith("*") else want[c])
        # the decode entry's prototype, then window and sinks
        assert args == L.DECODE_SIGNATURES[name[:-len("_window")]][1] + [ctypes.c_int, ctypes.c_void_p]
        fn = getattr(L.lib(), name)
        assert fn.restype is res and fn.argtypes == args
    assert len(L.SIGNATURES) == 69 and L.lib().sage_abi_version() == 3        # the core header is what it was


@pytest.mark.parametrize("rows", [False, True])
def test_refusals(rows):
    """raised before any device call (the tensors are on the CPU), in the words of window.py where it has them"""
    import sageattention_amd as sa
    assert {"sageattn_decode_paged_window", "sageattn_decode_paged_window_compilable"} <= set(sa.__all__)
    cache = _cpu_whole(rows=rows)                                                 # 3 sequences, Hk = 2, head_dim 64
    table, lens = torch.zeros(3, 3, dtype=torch.int32), torch.tensor([80, 3, 0], dtype=torch.int32)
    q = torch.zeros(3, 2, 8, 64, dtype=torch.float16)
    f = lambda window, qq=q, c=cache, **kw: sa.sageattn_decode_paged_window(qq, c, table, lens, window, q_fold=4, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="at most 32 query rows.*sageattn_splitkv_paged_window"):
        f(7, torch.zeros(3, 2, 36, 64, dtype=torch.float16))
    for args, kw, exc in (((0,), {}, ValueError), ((2.0,), {}, TypeError), ((7,), {"sinks": torch.zeros(3)}, ValueError),
                          ((7,), {"sinks": torch.zeros(8, dtype=torch.float16)}, TypeError),
                          ((7,), {"sinks": torch.zeros(8, device="meta")}, ValueError),
                          ((7,), {"c": sa.SagePagedKVCacheV4(cache, None, None)}, TypeError), ((7,), {"num_splits": 17}, ValueError)):
        with pytest.raises(exc) as mine:
            f(*args, **kw)
        with pytest.raises(exc) as parents:
            sa.sageattn_splitkv_paged_window(q, kw.pop("c", cache), table, lens, *args, q_fold=4, **kw)
        assert str(mine.value) == str(parents.value)


def test_ops_and_fake_shapes():
    import sageattention_amd  # noqa: F401
    ops = getattr(torch.ops, NS)
    names = ["attn_decode_paged_window", "attn_decode_paged_window_lse"]
    assert sorted(n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith(NS + "::")) == names
    schema = ("(Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor block_table, Tensor kv_lens, "
              "SymInt num_splits, SymInt q_fold, SymInt window, Tensor? sinks, str tensor_layout, float sm_scale, str qk_quant_gran)")
    for name, ret in zip(names, ("Tensor", "(Tensor, Tensor)")):
        assert str(getattr(ops, name).default._schema) == f"{NS}::{name}{schema} -> {ret}"
    for layout, shape in (("HND", (3, 2, 12, 64)), ("NHD", (3, 12, 2, 64))):
        c = _cpu_whole(layout=layout)
        q = torch.empty(shape, dtype=torch.float16, device="meta")
        args = [t.to("meta") for t in (c.k8, c.k_scale, c.km, c.v)] + [None, torch.empty(3, 3, dtype=torch.int32, device="meta"),
                                                                        torch.empty(3, dtype=torch.int32, device="meta")]
        sinks = torch.empty(8, device="meta")
        o, lse = ops.attn_decode_paged_window_lse(q, *args, 0, 4, 100, sinks, layout, 0.125, "per_thread")
        assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == (3, 2, 12) and lse.dtype == torch.float32
        assert ops.attn_decode_paged_window(q, *args, 1, 4, 100, None, layout, 0.125, "per_thread").shape == q.shape
