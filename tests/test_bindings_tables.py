"""The two tables the Python side is generated from: ``_lib.SIGNATURES`` (the ctypes signature of every C symbol) against the
prototypes of include/sageattn_hip.h, and ``ops._OPS`` (the torch.library ops) against the schemas they have always had, what
their fakes describe, and -- on the GPU -- the core operator each one forwards to."""
import ctypes
import json
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.utils._python_dispatch import TorchDispatchMode

import sageattention_amd.ops as ops
from sageattention_amd import _lib as L
from sageattention_amd import core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMAS = json.load(open(os.path.join(ROOT, "tests", "golden", "op_schemas.json")))
NS = torch.ops.sageattention_amd

# ---- _lib.SIGNATURES against the header --------------------------------------------------------------------------------
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "sage_stream_t": ctypes.c_void_p, "char*": ctypes.c_char_p}
_STRUCTS = {"sage_tensor*": L.SageTensor, "sage_op_opts*": L.OpOpts, "sage_kv_layout*": L.KvLayout}
_POINTEES = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
             "uint8_t": ctypes.c_uint8, "void": None, "void*": ctypes.c_void_p, "float*": ctypes.POINTER(ctypes.c_float)}


def _prototypes():
    """name -> (return type, [parameter types]) of every function include/sageattn_hip.h declares, as C type strings without
    ``const`` and spaces"""
    text = open(os.path.join(ROOT, "include", "sageattn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    ctype = lambda s: re.sub(r"\bconst\b|\s", "", s)  # noqa: E731
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(sage_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [p.strip() for p in params.split(",")]
        params = [] if params in ([""], ["void"]) else [ctype(re.sub(r"\w+$", "", p)) for p in params]
        assert name not in out and all(params), name
        out[name] = (ctype(ret), params)
    return out


def _agrees(c, ct):
    """does the ctypes type ``ct`` bind the C type ``c``?"""
    if c in _SCALARS:
        return ct is _SCALARS[c]
    if c in _STRUCTS:
        return ct is ctypes.POINTER(_STRUCTS[c])
    if c.endswith("*") and c[:-1] in _POINTEES:  # any other pointer: untyped, or typed by its pointee
        pointee = _POINTEES[c[:-1]]
        return ct is ctypes.c_void_p or (pointee is not None and ct is ctypes.POINTER(pointee))
    return False


def test_bindings_match_header():
    protos = _prototypes()
    assert sorted(protos) == sorted(L.SIGNATURES) and len(protos) == 69
    wrong = []
    for name, (ret, params) in protos.items():
        res, args = L.SIGNATURES[name]
        if not _agrees(ret, res) or len(params) != len(args):
            wrong.append((name, ret, len(params), res, len(args)))
        wrong += [(name, i, c, ct) for i, (c, ct) in enumerate(zip(params, args)) if not _agrees(c, ct)]
    assert not wrong, wrong


# ---- ops._OPS ----------------------------------------------------------------------------------------------------------------
def _registered():
    return sorted(n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith("sageattention_amd::"))


def test_op_schemas_are_the_parents():
    """tests/golden/op_schemas.json was written from the commit before the ops were generated from a table, by

        import json, torch, sageattention_amd.ops
        ns = torch.ops.sageattention_amd
        names = sorted(n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith("sageattention_amd::"))
        json.dump({n: str(getattr(ns, n).default._schema) for n in names}, open("tests/golden/op_schemas.json", "w"),
                  indent=1, sort_keys=True)
    """
    assert len(SCHEMAS) == 26 and _registered() == sorted(SCHEMAS)
    assert {n: str(getattr(NS, n).default._schema) for n in SCHEMAS} == SCHEMAS
    assert all(getattr(ops, n)._opoverload is getattr(NS, n).default for n in SCHEMAS)   # ops.attn, ops.attn_lse, ...


B, HQ, HK, M, N, D = 2, 2, 1, 130, 200, 64   # two q-blocks, the second ragged; four key tiles, the last ragged
NQB, NKT = (M + 127) // 128, (N + 63) // 64


def _qkv(layout, make):
    shape = lambda h, n: (B, h, n, D) if layout == "HND" else (B, n, h, D)  # noqa: E731
    return make(shape(HQ, M)), make(shape(HK, N)), make(shape(HK, N))


def _expected_outputs(name, q, outs):
    """count, shape, dtype and contiguous strides of what the op ``name`` returns for q [B,HQ,M,D] (either layout)"""
    outs = outs if isinstance(outs, tuple) else (outs,)
    want = [(q.shape, q.dtype)]
    want += [((B, HQ, M), torch.float32)] * ("_lse" in name) + [((B, HQ, NQB, 4), torch.int32)] * ("_pv" in name)
    assert len(outs) == len(want), (name, len(outs))
    for t, (shape, dtype) in zip(outs, want):
        assert tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.is_contiguous() and t.device == q.device, name
    return [(tuple(t.shape), t.dtype, t.stride()) for t in outs]


@pytest.mark.parametrize("layout", ["HND", "NHD"])
def test_every_fake_describes_its_outputs(layout):
    with FakeTensorMode():
        cuda = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda")  # noqa: E731
        q, k, v = _qkv(layout, lambda s: cuda(s, torch.float16))
        per_head = cuda((HQ,), torch.float32)
        values = dict(q=q, k=k, v=v, block_map=cuda((B, HQ, NQB, NKT), torch.bool), block_lists=cuda((64,), torch.int32),
                      plan_shape=[B, HQ, M, N], pvthreshd=per_head, kv_lens=cuda((B,), torch.int32), simthreshd1=per_head,
                      cdfthreshd=per_head, rule_param=per_head, rule="topk", keep_first=1, keep_last=0, num_splits=2, q_fold=2,
                      tensor_layout=layout, is_causal=False, sm_scale=0.125, pv="fp16", qk_quant_gran="per_thread")
        for name in SCHEMAS:
            op = getattr(NS, name)
            args = [values[a.name] for a in op.default._schema.arguments]
            _expected_outputs(name, q, op(*args))
            _expected_outputs(name, q, op(*args[:3], **{a.name: values[a.name] for a in op.default._schema.arguments[3:]}))


# ---- every op through its wrapper, on the GPU ------------------------------------------------------------------------------
class _OpsCalled(TorchDispatchMode):
    """the ops of this package that reach the dispatcher"""

    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func.namespace == "sageattention_amd":
            self.names.append(func._schema.name.split("::")[1])
        return func(*args, **(kwargs or {}))


NHD_ONCE = {"attn_lse", "attn_kvlen_lse", "attn_block_sparse_plan_pv_kvlen", "attn_sparge_pv_lse_kvlen", "attn_splitkv_lse",
            "attn_splitkv_causal_lse"}   # one op of every family runs in the other layout


@pytest.fixture(scope="module")
def operands():
    """q, k, v per layout (the NHD ones are the same values transposed), the lengths, the block map and its plan; read-only"""
    g = torch.Generator().manual_seed(0)
    hnd = _qkv("HND", lambda s: torch.randn(s, generator=g, dtype=torch.float16).cuda())
    block_map = torch.rand(B, HQ, NQB, NKT, generator=g) < 0.5
    block_map[..., 0] = True
    block_map = block_map.cuda()
    return {"HND": hnd, "NHD": tuple(t.transpose(1, 2).contiguous() for t in hnd),
            "kv_lens": torch.tensor([200, 70], dtype=torch.int32, device="cuda"), "block_map": block_map,
            "plan": core.block_sparse_plan(block_map, M, N)}


def _case(name, operands):
    """-> (the wrapper that reaches the op ``name``, the core operator behind it, the keywords both take: tensors, others)"""
    tensors, kw = {}, {"return_lse": True} if "_lse" in name else {}
    if "_kvlen" in name or "splitkv" in name:
        tensors["kv_lens"] = operands["kv_lens"]
    if "_pv" in name:
        kw.update(pvthreshd=4.0, return_skipped=True)
    if name.startswith("attn_block_sparse"):
        wrapper, operator = ops.sageattn_block_sparse_compilable, core.sageattn_block_sparse
        (kw if "_plan" in name else tensors)["block_map"] = operands["plan" if "_plan" in name else "block_map"]
    elif name.startswith("attn_sparge"):
        wrapper, operator = ops.sageattn_sparge_compilable, core.sageattn_sparge
        if name not in ("attn_sparge", "attn_sparge_lse"):
            kw.update(topk=0.5, keep_first=1)
    elif name.startswith("attn_splitkv_causal"):
        wrapper, operator = ops.sageattn_splitkv_causal_compilable, core.sageattn_splitkv_causal
        kw.update(num_splits=2, q_fold=2)   # 65 tokens of two rows
    elif name.startswith("attn_splitkv"):
        wrapper, operator = ops.sageattn_splitkv_compilable, core.sageattn_splitkv
        kw.update(num_splits=2)
    elif name.startswith("attn_kvlen"):
        wrapper, operator = ops.sageattn_kvlen_compilable, core.sageattn_kvlen
    else:
        wrapper, operator = (lambda *a, **k: ops.sageattn_compilable(*a, pv="fp16", **k)), core.sageattn_qk_int8_pv_fp16_cuda
    return wrapper, operator, tensors, kw


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_every_op_matches_its_operator(name, operands):
    layout = "NHD" if name in NHD_ONCE else "HND"
    q, k, v = operands[layout]
    wrapper, operator, tensors, kw = _case(name, operands)
    kw["tensor_layout"] = layout
    as_tuple = lambda x: x if isinstance(x, tuple) else (x,)  # noqa: E731
    want = as_tuple(operator(q, k, v, **tensors, **kw))
    with _OpsCalled() as called:
        eager = as_tuple(wrapper(q, k, v, **tensors, **kw))
    assert called.names == [name]
    torch.compiler.reset()   # the lambda below is one code object for all 26 cases: without this, the recompile limit
    compiled = as_tuple(torch.compile(lambda a, b, c, t: wrapper(a, b, c, **t, **kw), backend="aot_eager",
                                      fullgraph=True)(q, k, v, tensors))
    torch.cuda.synchronize()
    for got in (eager, compiled):
        assert len(got) == len(want) and all(torch.equal(x, y) for x, y in zip(got, want))
    with FakeTensorMode() as mode:
        fq, fk, fv = (mode.from_tensor(t) for t in (q, k, v))
        fake_kw = {n: mode.from_tensor(t) for n, t in tensors.items()}
        if "_plan" in name:
            plan = kw["block_map"]
            fake_kw["block_map"] = core.BlockSparsePlan(mode.from_tensor(plan.lists), plan.B, plan.Hq, plan.M, plan.N)
        fake = wrapper(fq, fk, fv, **{**kw, **fake_kw})
    assert _expected_outputs(name, q, fake) == [(tuple(t.shape), t.dtype, t.stride()) for t in eager]
