"""``torch.library`` registration of the operator, so that ``torch.compile`` traces THROUGH a model that calls it
instead of breaking the graph.  The reference marks every entry point ``@torch.compiler.disable``
(core.py:160,362,479,655,907), which forces a graph break around each attention call.

Every op is ``torch.ops.sageattention_amd.<name>(q, k, v, <its own arguments>, tensor_layout, [is_causal,] sm_scale, pv,
qk_quant_gran)`` and returns o, then lse, then the skip counters, each if the op has it.  ``_OPS`` below is the list: one row
per op, registered by one loop with one body and one fake.  The families and the suffixes that multiply them:

    attn, attn_kvlen                      the dense operator; with per-batch key lengths (kv_lens int32 [B], on the device)
    attn_block_sparse[_plan]              a block map tensor, or a compacted plan as (block_lists, plan_shape)
    attn_sparge                           the block map predicted from q and k: (simthreshd1, cdfthreshd), fp32 [Hq] tensors
    attn_sparge_select, attn_sparge_pv    ... with the rule named ("cdf" | "topk": rule_param) and key blocks pinned on
    attn_splitkv[_causal]                 split-KV: kv_lens an optional tensor, num_splits 0 = automatic; causal for the chunk
                                          at the end of the keys, q_fold (a SymInt) query rows per token
    _lse      also returns lse            _pv     the P.V skip: the per-head threshold tensor in, the skip counters out
    _kvlen    kv_lens in front of the layout (block-sparse and Sparge ops)

The bodies call the same host code as ``sageattn_qk_int8_pv_{fp16,fp8}_cuda`` (core.py) and therefore the same HIP
kernels; the fake (meta) implementations only describe shapes, dtypes and strides.  ``sageattn_compilable`` is the
keyword-friendly wrapper with the reference's signature."""
from typing import Any, Optional

import torch

from . import core

__all__ = ["sageattn_compilable", "sageattn_block_sparse_compilable", "sageattn_sparge_compilable",
           "sageattn_kvlen_compilable", "sageattn_splitkv_compilable", "sageattn_splitkv_causal_compilable"]


def _entry(pv: str):
    if pv == "fp16":
        return core.sageattn_qk_int8_pv_fp16_cuda
    if pv == "fp8":
        return core.sageattn_qk_int8_pv_fp8_cuda
    raise ValueError(f"Unknown pv: {pv}")


def _bhm(q, tensor_layout):
    """(B, Hq, M) of q in either layout"""
    return (q.shape[0], q.shape[1], q.shape[2]) if tensor_layout == "HND" else (q.shape[0], q.shape[2], q.shape[1])


def _lse_like(q, tensor_layout):
    return q.new_empty(_bhm(q, tensor_layout), dtype=torch.float32)


def _skipped_like(q, tensor_layout):
    """the skip counters of a call on q: int32 [B, Hq, ceil(M/128), 4]"""
    B, H, M = _bhm(q, tensor_layout)
    return q.new_empty((B, H, (M + 127) // 128, 4), dtype=torch.int32)


def _as_per_head(value, q, tensor_layout):
    """a per-head parameter as the fp32 [Hq] tensor the ops take: a float is broadcast, a tensor passed on"""
    if isinstance(value, torch.Tensor):
        return value
    return torch.full((_bhm(q, tensor_layout)[1],), float(value), dtype=torch.float32, device=q.device)


def _plan_args(plan):
    """a plan as it travels through an op: its lists and the (B, Hq, M, N) it was compacted for, which the operator checks
    against the call"""
    return plan.lists, [plan.B, plan.Hq, plan.M, plan.N]


def _select_kwargs(rule_param: torch.Tensor, rule: str):
    if rule not in ("cdf", "topk"):
        raise ValueError(f"rule must be 'cdf' or 'topk', got {rule}")
    return {"topk": rule_param} if rule == "topk" else {"cdfthreshd": rule_param}


def _check_layout(tensor_layout):
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")


# The schema arguments an op has between (q, k, v) and the tail.  Thresholds travel as fp32 [Hq] tensors: per-head values are
# tensors anyway, and a float is broadcast by the wrapper.
_MAP, _PLAN = "Tensor block_map", "Tensor block_lists, SymInt[] plan_shape"
_PVT, _KVL = "Tensor pvthreshd", "Tensor kv_lens"
_CDF = "Tensor simthreshd1, Tensor cdfthreshd"
_SEL = "Tensor simthreshd1, Tensor rule_param, str rule, SymInt keep_first, SymInt keep_last"
_SPLIT = "Tensor? kv_lens, SymInt num_splits"
_TAKES_IS_CAUSAL = (None, "sageattn_kvlen")

# (op, the core operator it calls -- None: the dense entry its pv names, its own arguments, its outputs).  A new form is an op
# of its own, so that the schemas of the others stay as they are.
_OPS = (
    ("attn", None, "", "o"),
    ("attn_lse", None, "", "o lse"),
    ("attn_kvlen", "sageattn_kvlen", _KVL, "o"),
    ("attn_kvlen_lse", "sageattn_kvlen", _KVL, "o lse"),
    ("attn_block_sparse", "sageattn_block_sparse", _MAP, "o"),
    ("attn_block_sparse_plan", "sageattn_block_sparse", _PLAN, "o"),
    ("attn_block_sparse_pv", "sageattn_block_sparse", f"{_MAP}, {_PVT}", "o skipped"),
    ("attn_block_sparse_plan_pv", "sageattn_block_sparse", f"{_PLAN}, {_PVT}", "o skipped"),
    ("attn_block_sparse_kvlen", "sageattn_block_sparse", f"{_MAP}, {_KVL}", "o"),
    ("attn_block_sparse_plan_kvlen", "sageattn_block_sparse", f"{_PLAN}, {_KVL}", "o"),
    ("attn_block_sparse_pv_kvlen", "sageattn_block_sparse", f"{_MAP}, {_PVT}, {_KVL}", "o skipped"),
    ("attn_block_sparse_plan_pv_kvlen", "sageattn_block_sparse", f"{_PLAN}, {_PVT}, {_KVL}", "o skipped"),
    ("attn_sparge", "sageattn_sparge", _CDF, "o"),
    ("attn_sparge_lse", "sageattn_sparge", _CDF, "o lse"),
    ("attn_sparge_select", "sageattn_sparge", _SEL, "o"),
    ("attn_sparge_select_lse", "sageattn_sparge", _SEL, "o lse"),
    ("attn_sparge_pv", "sageattn_sparge", f"{_SEL}, {_PVT}", "o skipped"),
    ("attn_sparge_pv_lse", "sageattn_sparge", f"{_SEL}, {_PVT}", "o lse skipped"),
    ("attn_sparge_select_kvlen", "sageattn_sparge", f"{_SEL}, {_KVL}", "o"),
    ("attn_sparge_select_lse_kvlen", "sageattn_sparge", f"{_SEL}, {_KVL}", "o lse"),
    ("attn_sparge_pv_kvlen", "sageattn_sparge", f"{_SEL}, {_PVT}, {_KVL}", "o skipped"),
    ("attn_sparge_pv_lse_kvlen", "sageattn_sparge", f"{_SEL}, {_PVT}, {_KVL}", "o lse skipped"),
    ("attn_splitkv", "sageattn_splitkv", _SPLIT, "o"),
    ("attn_splitkv_lse", "sageattn_splitkv", _SPLIT, "o lse"),
    ("attn_splitkv_causal", "sageattn_splitkv_causal", f"{_SPLIT}, SymInt q_fold", "o"),
    ("attn_splitkv_causal_lse", "sageattn_splitkv_causal", f"{_SPLIT}, SymInt q_fold", "o lse"),
)
_LIKE = {"o": lambda q, tensor_layout: q.new_empty(q.shape), "lse": _lse_like, "skipped": _skipped_like}


def _register(name, operator, own, outputs):
    outputs = outputs.split()
    tail = ("str tensor_layout", "bool is_causal" * (operator in _TAKES_IS_CAUSAL), "float sm_scale, str pv, str qk_quant_gran")
    params = ", ".join(filter(None, ("Tensor q, Tensor k, Tensor v", own, *tail)))
    returns = "Tensor" if len(outputs) == 1 else "(" + ", ".join(["Tensor"] * len(outputs)) + ")"
    own_names = [p.split()[-1] for p in params.split(", ")][3:]   # bound by name, so that keyword calls work
    flags = {"return_" + o: True for o in outputs[1:]}             # return_lse, return_skipped
    has_plan, has_map, has_rule, has_splits = (n in own_names for n in ("block_lists", "block_map", "rule", "num_splits"))

    def body(q, k, v, *args, **kwargs):
        a = dict(zip(own_names, args), **kwargs, **flags)
        fn = _entry(a.pop("pv")) if operator is None else getattr(core, operator)
        if has_rule:
            a.update(_select_kwargs(a.pop("rule_param"), a.pop("rule")))
        if has_splits:
            a["num_splits"] = a["num_splits"] or None
        if has_plan:
            out = fn(q, k, v, core.BlockSparsePlan(a.pop("block_lists"), *(int(x) for x in a.pop("plan_shape"))), **a)
        elif has_map:
            out = fn(q, k, v, a.pop("block_map"), **a)
        else:
            out = fn(q, k, v, **a)
        # a contiguous o whatever the inputs' strides / head-dim padding: the fake implementation below must describe exactly
        # the layout the real op returns, or Inductor indexes the output with the wrong strides
        return (out[0].contiguous(), *out[1:]) if flags else out.contiguous()

    def fake(q, k, v, *args, **kwargs):
        tensor_layout = dict(zip(own_names, args), **kwargs)["tensor_layout"]
        out = tuple(_LIKE[o](q, tensor_layout) for o in outputs)
        return out if flags else out[0]

    op = torch.library.custom_op(f"sageattention_amd::{name}", body, mutates_args=(), schema=f"({params}) -> {returns}")
    op.register_fake(fake)
    return op


for _row in _OPS:
    globals()[_row[0]] = _register(*_row)   # ops.attn, ops.attn_lse, ...
_NS = torch.ops.sageattention_amd


def sageattn_block_sparse_compilable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_map,
                                     tensor_layout: str = "HND", sm_scale: Optional[float] = None, pv: str = "fp16",
                                     qk_quant_gran: str = "per_thread", pvthreshd=None, return_skipped: bool = False,
                                     kv_lens: Optional[torch.Tensor] = None):
    """``sageattn_block_sparse`` (core.py) as a traceable custom op; ``block_map`` is the map tensor or a plan.  With
    ``pvthreshd`` (a float > 0 or an fp32 tensor [Hq]) it calls the ``_pv`` ops, and ``return_skipped`` appends the skip
    counters; without it the ops it has always called.  With ``kv_lens`` (int32 [B], per-batch key lengths) the ``_kvlen``
    twin of the op it would call without."""
    _check_layout(tensor_layout)
    core._check_pvskip_args(pvthreshd, return_skipped)
    if sm_scale is None:
        sm_scale = q.size(-1) ** -0.5
    is_plan = isinstance(block_map, core.BlockSparsePlan)
    own = list(_plan_args(block_map)) if is_plan else [block_map]
    if pvthreshd is not None:
        own.append(_as_per_head(pvthreshd, q, tensor_layout))
    if kv_lens is not None:
        own.append(kv_lens)
    name = "attn_block_sparse" + "_plan" * is_plan + "_pv" * (pvthreshd is not None) + "_kvlen" * (kv_lens is not None)
    out = getattr(_NS, name)(q, k, v, *own, tensor_layout, float(sm_scale), pv, qk_quant_gran)
    return out if pvthreshd is None or return_skipped else out[0]


def sageattn_sparge_compilable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tensor_layout: str = "HND",
                               simthreshd1=0.6, cdfthreshd=0.98, sm_scale: Optional[float] = None, pv: str = "fp16",
                               qk_quant_gran: str = "per_thread", return_lse: bool = False, topk=None,
                               keep_first: int = 0, keep_last: int = 0, pvthreshd=None, return_skipped: bool = False,
                               kv_lens: Optional[torch.Tensor] = None):
    """``sageattn_sparge`` (core.py) as a traceable custom op; thresholds and ``topk`` are floats or fp32 tensors [Hq].
    With ``topk`` the budget rule is used and ``cdfthreshd`` is not read; ``keep_first`` / ``keep_last`` pin key blocks on.
    Without any of the three it calls ``attn_sparge`` / ``attn_sparge_lse`` as before, otherwise the ``attn_sparge_select``
    pair.  With ``pvthreshd`` (a float > 0 or an fp32 tensor [Hq]) it calls the ``attn_sparge_pv`` pair, and
    ``return_skipped`` appends the skip counters: o, lse, skipped.  With ``kv_lens`` (int32 [B], per-batch key lengths) it
    calls the ``_kvlen`` twins of the ``attn_sparge_select`` and ``attn_sparge_pv`` pairs."""
    _check_layout(tensor_layout)
    core._check_select_args(topk, keep_first, keep_last)
    core._check_pvskip_args(pvthreshd, return_skipped)
    if sm_scale is None:
        sm_scale = q.size(-1) ** -0.5
    rule, par = ("cdf", cdfthreshd) if topk is None else ("topk", topk)
    own = [_as_per_head(simthreshd1, q, tensor_layout), _as_per_head(par, q, tensor_layout)]
    if pvthreshd is None and kv_lens is None and topk is None and keep_first == 0 and keep_last == 0:
        name = "attn_sparge"
    else:
        name = "attn_sparge_select" if pvthreshd is None else "attn_sparge_pv"
        own += [rule, keep_first, keep_last]
    if pvthreshd is not None:
        own.append(_as_per_head(pvthreshd, q, tensor_layout))
    op = getattr(_NS, name + "_lse" * bool(return_lse) + "_kvlen" * (kv_lens is not None))
    if kv_lens is not None:
        own.append(kv_lens)
    out = op(q, k, v, *own, tensor_layout, float(sm_scale), pv, qk_quant_gran)
    if pvthreshd is None:
        return out
    out = out if return_skipped else out[:-1]
    return out if len(out) > 1 else out[0]


def sageattn_kvlen_compilable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_lens: torch.Tensor,
                              tensor_layout: str = "HND", is_causal: bool = False, sm_scale: Optional[float] = None,
                              pv: str = "fp16", qk_quant_gran: str = "per_thread", return_lse: bool = False):
    """``sageattn_kvlen`` (core.py) as a traceable custom op: ``kv_lens`` is the int32 [B] tensor of valid keys per batch."""
    _check_layout(tensor_layout)
    if sm_scale is None:
        sm_scale = q.size(-1) ** -0.5
    op = _NS.attn_kvlen_lse if return_lse else _NS.attn_kvlen
    return op(q, k, v, kv_lens, tensor_layout, bool(is_causal), float(sm_scale), pv, qk_quant_gran)


def _splitkv_compilable_args(q, tensor_layout, num_splits, sm_scale):
    """what the two split-KV wrappers below check, and the op's forms of num_splits (0: automatic) and sm_scale"""
    _check_layout(tensor_layout)
    if num_splits is not None and not 1 <= int(num_splits) <= core.SPLITKV_MAX:
        raise ValueError(f"num_splits must be in [1, {core.SPLITKV_MAX}] (or None: from the shape), got {num_splits}")
    return int(num_splits or 0), float(q.size(-1) ** -0.5 if sm_scale is None else sm_scale)


def sageattn_splitkv_compilable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_lens: Optional[torch.Tensor] = None,
                                num_splits: Optional[int] = None, tensor_layout: str = "HND",
                                sm_scale: Optional[float] = None, pv: str = "fp16", qk_quant_gran: str = "per_thread",
                                return_lse: bool = False):
    """``sageattn_splitkv`` (core.py) as a traceable custom op: ``kv_lens`` is an optional int32 [B] tensor argument of the op,
    ``num_splits`` an int with 0 for the automatic choice (``core.splitkv_num_splits``)."""
    num_splits, sm_scale = _splitkv_compilable_args(q, tensor_layout, num_splits, sm_scale)
    op = _NS.attn_splitkv_lse if return_lse else _NS.attn_splitkv
    return op(q, k, v, kv_lens, num_splits, tensor_layout, sm_scale, pv, qk_quant_gran)


def sageattn_splitkv_causal_compilable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                       kv_lens: Optional[torch.Tensor] = None, num_splits: Optional[int] = None,
                                       q_fold: int = 1, tensor_layout: str = "HND", sm_scale: Optional[float] = None,
                                       pv: str = "fp16", qk_quant_gran: str = "per_thread", return_lse: bool = False):
    """``sageattn_splitkv_causal`` (core.py) as a traceable custom op: ``kv_lens`` is an optional int32 [B] tensor argument of
    the op, ``num_splits`` an int with 0 for the automatic choice (``core.splitkv_num_splits``), ``q_fold`` the query rows per
    token."""
    num_splits, sm_scale = _splitkv_compilable_args(q, tensor_layout, num_splits, sm_scale)
    op = _NS.attn_splitkv_causal_lse if return_lse else _NS.attn_splitkv_causal
    return op(q, k, v, kv_lens, num_splits, q_fold, tensor_layout, sm_scale, pv, qk_quant_gran)


def sageattn_compilable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tensor_layout: str = "HND",
                        is_causal: bool = False, sm_scale: Optional[float] = None, return_lse: bool = False,
                        pv: str = "auto", qk_quant_gran: str = "per_thread", **kwargs: Any):
    """``sageattn`` (core.py:80-144) as a traceable custom op.  ``pv="auto"`` follows the dispatcher of the package
    (``core.dispatch_pv``: FP8 PV from a few thousand keys per row upwards, FP16 PV below; per_thread scales); unknown
    keyword arguments are accepted and ignored like there."""
    _check_layout(tensor_layout)
    if pv == "auto":
        pv = core.dispatch_pv(q, k, tensor_layout, bool(is_causal))
    if sm_scale is None:
        sm_scale = q.size(-1) ** -0.5
    op = _NS.attn_lse if return_lse else _NS.attn
    return op(q, k, v, tensor_layout, bool(is_causal), float(sm_scale), pv, qk_quant_gran)
