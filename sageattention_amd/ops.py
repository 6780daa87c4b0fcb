"""``torch.library`` registration of the operator, so that ``torch.compile`` traces THROUGH a model that calls it
instead of breaking the graph.  The reference marks every entry point ``@torch.compiler.disable``
(core.py:160,362,479,655,907), which forces a graph break around each attention call.

    torch.ops.sageattention_amd.attn(q, k, v, tensor_layout, is_causal, sm_scale, pv, qk_quant_gran) -> o
    torch.ops.sageattention_amd.attn_lse(...) -> (o, lse)
    torch.ops.sageattention_amd.attn_block_sparse(q, k, v, block_map, tensor_layout, sm_scale, pv, qk_quant_gran) -> o
    torch.ops.sageattention_amd.attn_block_sparse_plan(q, k, v, block_lists, plan_shape, ...) -> o   (a compacted plan)
    torch.ops.sageattention_amd.attn_sparge(q, k, v, simthreshd1, cdfthreshd, tensor_layout, sm_scale, pv, qk_quant_gran) -> o
    torch.ops.sageattention_amd.attn_sparge_lse(...) -> (o, lse)          (the block map predicted from q and k)
    torch.ops.sageattention_amd.attn_sparge_select(q, k, v, simthreshd1, rule_param, rule, keep_first, keep_last, tensor_layout,
                                                   sm_scale, pv, qk_quant_gran) -> o      (rule "cdf" | "topk", kept key blocks)
    torch.ops.sageattention_amd.attn_sparge_select_lse(...) -> (o, lse)
    torch.ops.sageattention_amd.attn_block_sparse_pv(q, k, v, block_map, pvthreshd, ...) -> (o, skipped)   (the P.V skip: the
    torch.ops.sageattention_amd.attn_block_sparse_plan_pv(q, k, v, block_lists, plan_shape, pvthreshd, ...)  per-head threshold
    torch.ops.sageattention_amd.attn_sparge_pv(q, k, v, simthreshd1, rule_param, rule, keep_first, keep_last, pvthreshd, ...)
    torch.ops.sageattention_amd.attn_sparge_pv_lse(...) -> (o, lse, skipped)        tensor in, the skip counters out)
    torch.ops.sageattention_amd.attn_kvlen(q, k, v, kv_lens, tensor_layout, is_causal, sm_scale, pv, qk_quant_gran) -> o
    torch.ops.sageattention_amd.attn_kvlen_lse(...) -> (o, lse)           (per-batch key lengths, int32 [B] on the device)
    torch.ops.sageattention_amd.attn_block_sparse_kvlen(q, k, v, block_map, kv_lens, ...) -> o      (the block-sparse and Sparge
    torch.ops.sageattention_amd.attn_block_sparse_plan_kvlen(q, k, v, block_lists, plan_shape, kv_lens, ...) -> o    ops with
    torch.ops.sageattention_amd.attn_block_sparse_pv_kvlen / attn_block_sparse_plan_pv_kvlen(...) -> (o, skipped)   per-batch
    torch.ops.sageattention_amd.attn_sparge_select_kvlen(q, k, v, simthreshd1, rule_param, rule, keep_first,       key lengths:
                                                         keep_last, kv_lens, ...) -> o             kv_lens in front of the layout)
    torch.ops.sageattention_amd.attn_sparge_select_lse_kvlen(...) -> (o, lse)
    torch.ops.sageattention_amd.attn_sparge_pv_kvlen / attn_sparge_pv_lse_kvlen(..., pvthreshd, kv_lens, ...) -> (o, [lse,] skipped)
    torch.ops.sageattention_amd.attn_splitkv(q, k, v, kv_lens, num_splits, tensor_layout, sm_scale, pv, qk_quant_gran) -> o
    torch.ops.sageattention_amd.attn_splitkv_lse(...) -> (o, lse)   (split-KV: kv_lens an optional tensor, num_splits 0 = automatic)
    torch.ops.sageattention_amd.attn_splitkv_causal(q, k, v, kv_lens, num_splits, q_fold, tensor_layout, sm_scale, pv,
                                                    qk_quant_gran) -> o     (causal, the chunk at the end of the keys; q_fold
    torch.ops.sageattention_amd.attn_splitkv_causal_lse(...) -> (o, lse)     a SymInt: query rows per token)

The bodies call the same host code as ``sageattn_qk_int8_pv_{fp16,fp8}_cuda`` (core.py) and therefore the same HIP
kernels; the fake (meta) implementations only describe shapes, dtypes and strides.  ``sageattn_compilable`` is the
keyword-friendly wrapper with the reference's signature."""
from typing import Any, Optional, Sequence, Tuple

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


@torch.library.custom_op("sageattention_amd::attn", mutates_args=())
def attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tensor_layout: str, is_causal: bool, sm_scale: float,
         pv: str, qk_quant_gran: str) -> torch.Tensor:
    # contiguous result whatever the inputs' strides / head-dim padding: the fake implementation below must describe
    # exactly the layout the real op returns, or Inductor indexes the output with the wrong strides
    return _entry(pv)(q, k, v, tensor_layout=tensor_layout, is_causal=is_causal, sm_scale=sm_scale,
                      qk_quant_gran=qk_quant_gran).contiguous()


@attn.register_fake
def _(q, k, v, tensor_layout, is_causal, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape)


@torch.library.custom_op("sageattention_amd::attn_lse", mutates_args=())
def attn_lse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tensor_layout: str, is_causal: bool, sm_scale: float,
             pv: str, qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    o, lse = _entry(pv)(q, k, v, tensor_layout=tensor_layout, is_causal=is_causal, sm_scale=sm_scale,
                        qk_quant_gran=qk_quant_gran, return_lse=True)
    return o.contiguous(), lse


@attn_lse.register_fake
def _(q, k, v, tensor_layout, is_causal, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _lse_like(q, tensor_layout)


@torch.library.custom_op("sageattention_amd::attn_block_sparse", mutates_args=())
def attn_block_sparse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_map: torch.Tensor, tensor_layout: str,
                      sm_scale: float, pv: str, qk_quant_gran: str) -> torch.Tensor:
    return core.sageattn_block_sparse(q, k, v, block_map, tensor_layout=tensor_layout, sm_scale=sm_scale, pv=pv,
                                      qk_quant_gran=qk_quant_gran).contiguous()


@attn_block_sparse.register_fake
def _(q, k, v, block_map, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape)


@torch.library.custom_op("sageattention_amd::attn_block_sparse_plan", mutates_args=())
def attn_block_sparse_plan(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_lists: torch.Tensor,
                           plan_shape: Sequence[int], tensor_layout: str, sm_scale: float, pv: str,
                           qk_quant_gran: str) -> torch.Tensor:
    plan = core.BlockSparsePlan(block_lists, *(int(x) for x in plan_shape))
    return core.sageattn_block_sparse(q, k, v, plan, tensor_layout=tensor_layout, sm_scale=sm_scale, pv=pv,
                                      qk_quant_gran=qk_quant_gran).contiguous()


@attn_block_sparse_plan.register_fake
def _(q, k, v, block_lists, plan_shape, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape)


# ... with the P.V skip (core.sageattn_block_sparse, pvthreshd): ops of their own, so that the schemas above stay as they
# are.  The threshold travels as an fp32 [Hq] tensor and the skip counters are always returned.
@torch.library.custom_op("sageattention_amd::attn_block_sparse_pv", mutates_args=())
def attn_block_sparse_pv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_map: torch.Tensor, pvthreshd: torch.Tensor,
                         tensor_layout: str, sm_scale: float, pv: str, qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    o, skipped = core.sageattn_block_sparse(q, k, v, block_map, tensor_layout=tensor_layout, sm_scale=sm_scale, pv=pv,
                                            qk_quant_gran=qk_quant_gran, pvthreshd=pvthreshd, return_skipped=True)
    return o.contiguous(), skipped


@attn_block_sparse_pv.register_fake
def _(q, k, v, block_map, pvthreshd, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _skipped_like(q, tensor_layout)


@torch.library.custom_op("sageattention_amd::attn_block_sparse_plan_pv", mutates_args=())
def attn_block_sparse_plan_pv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_lists: torch.Tensor,
                              plan_shape: Sequence[int], pvthreshd: torch.Tensor, tensor_layout: str, sm_scale: float,
                              pv: str, qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    plan = core.BlockSparsePlan(block_lists, *(int(x) for x in plan_shape))
    o, skipped = core.sageattn_block_sparse(q, k, v, plan, tensor_layout=tensor_layout, sm_scale=sm_scale, pv=pv,
                                            qk_quant_gran=qk_quant_gran, pvthreshd=pvthreshd, return_skipped=True)
    return o.contiguous(), skipped


@attn_block_sparse_plan_pv.register_fake
def _(q, k, v, block_lists, plan_shape, pvthreshd, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _skipped_like(q, tensor_layout)


# ... with per-batch key lengths (core.sageattn_block_sparse, kv_lens): ops of their own again, so that the schemas above stay
# as they are.  kv_lens is the int32 [B] tensor, in front of the layout.
@torch.library.custom_op("sageattention_amd::attn_block_sparse_kvlen", mutates_args=())
def attn_block_sparse_kvlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_map: torch.Tensor, kv_lens: torch.Tensor,
                            tensor_layout: str, sm_scale: float, pv: str, qk_quant_gran: str) -> torch.Tensor:
    return core.sageattn_block_sparse(q, k, v, block_map, tensor_layout=tensor_layout, sm_scale=sm_scale, pv=pv,
                                      qk_quant_gran=qk_quant_gran, kv_lens=kv_lens).contiguous()


@attn_block_sparse_kvlen.register_fake
def _(q, k, v, block_map, kv_lens, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape)


@torch.library.custom_op("sageattention_amd::attn_block_sparse_plan_kvlen", mutates_args=())
def attn_block_sparse_plan_kvlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_lists: torch.Tensor,
                                 plan_shape: Sequence[int], kv_lens: torch.Tensor, tensor_layout: str, sm_scale: float,
                                 pv: str, qk_quant_gran: str) -> torch.Tensor:
    plan = core.BlockSparsePlan(block_lists, *(int(x) for x in plan_shape))
    return core.sageattn_block_sparse(q, k, v, plan, tensor_layout=tensor_layout, sm_scale=sm_scale, pv=pv,
                                      qk_quant_gran=qk_quant_gran, kv_lens=kv_lens).contiguous()


@attn_block_sparse_plan_kvlen.register_fake
def _(q, k, v, block_lists, plan_shape, kv_lens, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape)


@torch.library.custom_op("sageattention_amd::attn_block_sparse_pv_kvlen", mutates_args=())
def attn_block_sparse_pv_kvlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_map: torch.Tensor,
                               pvthreshd: torch.Tensor, kv_lens: torch.Tensor, tensor_layout: str, sm_scale: float, pv: str,
                               qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    o, skipped = core.sageattn_block_sparse(q, k, v, block_map, tensor_layout=tensor_layout, sm_scale=sm_scale, pv=pv,
                                            qk_quant_gran=qk_quant_gran, pvthreshd=pvthreshd, return_skipped=True,
                                            kv_lens=kv_lens)
    return o.contiguous(), skipped


@attn_block_sparse_pv_kvlen.register_fake
def _(q, k, v, block_map, pvthreshd, kv_lens, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _skipped_like(q, tensor_layout)


@torch.library.custom_op("sageattention_amd::attn_block_sparse_plan_pv_kvlen", mutates_args=())
def attn_block_sparse_plan_pv_kvlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_lists: torch.Tensor,
                                    plan_shape: Sequence[int], pvthreshd: torch.Tensor, kv_lens: torch.Tensor,
                                    tensor_layout: str, sm_scale: float, pv: str,
                                    qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    plan = core.BlockSparsePlan(block_lists, *(int(x) for x in plan_shape))
    o, skipped = core.sageattn_block_sparse(q, k, v, plan, tensor_layout=tensor_layout, sm_scale=sm_scale, pv=pv,
                                            qk_quant_gran=qk_quant_gran, pvthreshd=pvthreshd, return_skipped=True,
                                            kv_lens=kv_lens)
    return o.contiguous(), skipped


@attn_block_sparse_plan_pv_kvlen.register_fake
def _(q, k, v, block_lists, plan_shape, pvthreshd, kv_lens, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _skipped_like(q, tensor_layout)


def sageattn_block_sparse_compilable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_map,
                                     tensor_layout: str = "HND", sm_scale: Optional[float] = None, pv: str = "fp16",
                                     qk_quant_gran: str = "per_thread", pvthreshd=None, return_skipped: bool = False,
                                     kv_lens: Optional[torch.Tensor] = None):
    """``sageattn_block_sparse`` (core.py) as a traceable custom op; ``block_map`` is the map tensor or a plan.  With
    ``pvthreshd`` (a float > 0 or an fp32 tensor [Hq]) it calls the ``_pv`` ops, and ``return_skipped`` appends the skip
    counters; without it the ops it has always called.  With ``kv_lens`` (int32 [B], per-batch key lengths) the ``_kvlen``
    twin of the op it would call without."""
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")
    core._check_pvskip_args(pvthreshd, return_skipped)
    if sm_scale is None:
        sm_scale = q.size(-1) ** -0.5
    ns, tail = torch.ops.sageattention_amd, (tensor_layout, float(sm_scale), pv, qk_quant_gran)
    is_plan = isinstance(block_map, core.BlockSparsePlan)
    if kv_lens is not None:
        if pvthreshd is not None:
            thr = _as_per_head(pvthreshd, q, tensor_layout)
            if is_plan:
                o, skipped = ns.attn_block_sparse_plan_pv_kvlen(q, k, v, *_plan_args(block_map), thr, kv_lens, *tail)
            else:
                o, skipped = ns.attn_block_sparse_pv_kvlen(q, k, v, block_map, thr, kv_lens, *tail)
            return (o, skipped) if return_skipped else o
        if is_plan:
            return ns.attn_block_sparse_plan_kvlen(q, k, v, *_plan_args(block_map), kv_lens, *tail)
        return ns.attn_block_sparse_kvlen(q, k, v, block_map, kv_lens, *tail)
    if pvthreshd is not None:
        thr = _as_per_head(pvthreshd, q, tensor_layout)
        if is_plan:
            o, skipped = ns.attn_block_sparse_plan_pv(q, k, v, *_plan_args(block_map), thr, *tail)
        else:
            o, skipped = ns.attn_block_sparse_pv(q, k, v, block_map, thr, *tail)
        return (o, skipped) if return_skipped else o
    if is_plan:
        return ns.attn_block_sparse_plan(q, k, v, *_plan_args(block_map), *tail)
    return ns.attn_block_sparse(q, k, v, block_map, *tail)


@torch.library.custom_op("sageattention_amd::attn_sparge", mutates_args=())
def attn_sparge(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, simthreshd1: torch.Tensor, cdfthreshd: torch.Tensor,
                tensor_layout: str, sm_scale: float, pv: str, qk_quant_gran: str) -> torch.Tensor:
    # the thresholds travel as fp32 [Hq] tensors: per-head values are tensors anyway, and a float is broadcast by the wrapper
    return core.sageattn_sparge(q, k, v, tensor_layout=tensor_layout, simthreshd1=simthreshd1, cdfthreshd=cdfthreshd,
                                sm_scale=sm_scale, pv=pv, qk_quant_gran=qk_quant_gran).contiguous()


@attn_sparge.register_fake
def _(q, k, v, simthreshd1, cdfthreshd, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape)


@torch.library.custom_op("sageattention_amd::attn_sparge_lse", mutates_args=())
def attn_sparge_lse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, simthreshd1: torch.Tensor, cdfthreshd: torch.Tensor,
                    tensor_layout: str, sm_scale: float, pv: str, qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    o, lse = core.sageattn_sparge(q, k, v, tensor_layout=tensor_layout, simthreshd1=simthreshd1, cdfthreshd=cdfthreshd,
                                  sm_scale=sm_scale, pv=pv, qk_quant_gran=qk_quant_gran, return_lse=True)
    return o.contiguous(), lse


@attn_sparge_lse.register_fake
def _(q, k, v, simthreshd1, cdfthreshd, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _lse_like(q, tensor_layout)


def _select_kwargs(rule_param: torch.Tensor, rule: str):
    if rule not in ("cdf", "topk"):
        raise ValueError(f"rule must be 'cdf' or 'topk', got {rule}")
    return {"topk": rule_param} if rule == "topk" else {"cdfthreshd": rule_param}


@torch.library.custom_op("sageattention_amd::attn_sparge_select", mutates_args=())
def attn_sparge_select(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, simthreshd1: torch.Tensor, rule_param: torch.Tensor,
                       rule: str, keep_first: int, keep_last: int, tensor_layout: str, sm_scale: float, pv: str,
                       qk_quant_gran: str) -> torch.Tensor:
    # attn_sparge with the rule named ("cdf": rule_param = cdfthreshd, "topk": rule_param = topk) and key blocks pinned on
    return core.sageattn_sparge(q, k, v, tensor_layout=tensor_layout, simthreshd1=simthreshd1, sm_scale=sm_scale, pv=pv,
                                qk_quant_gran=qk_quant_gran, keep_first=keep_first, keep_last=keep_last,
                                **_select_kwargs(rule_param, rule)).contiguous()


@attn_sparge_select.register_fake
def _(q, k, v, simthreshd1, rule_param, rule, keep_first, keep_last, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape)


@torch.library.custom_op("sageattention_amd::attn_sparge_select_lse", mutates_args=())
def attn_sparge_select_lse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, simthreshd1: torch.Tensor,
                           rule_param: torch.Tensor, rule: str, keep_first: int, keep_last: int, tensor_layout: str,
                           sm_scale: float, pv: str, qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    o, lse = core.sageattn_sparge(q, k, v, tensor_layout=tensor_layout, simthreshd1=simthreshd1, sm_scale=sm_scale, pv=pv,
                                  qk_quant_gran=qk_quant_gran, return_lse=True, keep_first=keep_first, keep_last=keep_last,
                                  **_select_kwargs(rule_param, rule))
    return o.contiguous(), lse


@attn_sparge_select_lse.register_fake
def _(q, k, v, simthreshd1, rule_param, rule, keep_first, keep_last, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _lse_like(q, tensor_layout)


@torch.library.custom_op("sageattention_amd::attn_sparge_pv", mutates_args=())
def attn_sparge_pv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, simthreshd1: torch.Tensor, rule_param: torch.Tensor,
                   rule: str, keep_first: int, keep_last: int, pvthreshd: torch.Tensor, tensor_layout: str, sm_scale: float,
                   pv: str, qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    # attn_sparge_select with the P.V skip on the predicted tiles: the threshold tensor in, the skip counters out
    o, skipped = core.sageattn_sparge(q, k, v, tensor_layout=tensor_layout, simthreshd1=simthreshd1, sm_scale=sm_scale, pv=pv,
                                      qk_quant_gran=qk_quant_gran, keep_first=keep_first, keep_last=keep_last,
                                      pvthreshd=pvthreshd, return_skipped=True, **_select_kwargs(rule_param, rule))
    return o.contiguous(), skipped


@attn_sparge_pv.register_fake
def _(q, k, v, simthreshd1, rule_param, rule, keep_first, keep_last, pvthreshd, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _skipped_like(q, tensor_layout)


@torch.library.custom_op("sageattention_amd::attn_sparge_pv_lse", mutates_args=())
def attn_sparge_pv_lse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, simthreshd1: torch.Tensor, rule_param: torch.Tensor,
                       rule: str, keep_first: int, keep_last: int, pvthreshd: torch.Tensor, tensor_layout: str,
                       sm_scale: float, pv: str, qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    o, lse, skipped = core.sageattn_sparge(q, k, v, tensor_layout=tensor_layout, simthreshd1=simthreshd1, sm_scale=sm_scale,
                                           pv=pv, qk_quant_gran=qk_quant_gran, return_lse=True, keep_first=keep_first,
                                           keep_last=keep_last, pvthreshd=pvthreshd, return_skipped=True,
                                           **_select_kwargs(rule_param, rule))
    return o.contiguous(), lse, skipped


@attn_sparge_pv_lse.register_fake
def _(q, k, v, simthreshd1, rule_param, rule, keep_first, keep_last, pvthreshd, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _lse_like(q, tensor_layout), _skipped_like(q, tensor_layout)


# ... with per-batch key lengths (core.sageattn_sparge, kv_lens): the attn_sparge_select and attn_sparge_pv pairs again, kv_lens
# (int32 [B]) in front of the layout
@torch.library.custom_op("sageattention_amd::attn_sparge_select_kvlen", mutates_args=())
def attn_sparge_select_kvlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, simthreshd1: torch.Tensor,
                             rule_param: torch.Tensor, rule: str, keep_first: int, keep_last: int, kv_lens: torch.Tensor,
                             tensor_layout: str, sm_scale: float, pv: str, qk_quant_gran: str) -> torch.Tensor:
    return core.sageattn_sparge(q, k, v, tensor_layout=tensor_layout, simthreshd1=simthreshd1, sm_scale=sm_scale, pv=pv,
                                qk_quant_gran=qk_quant_gran, keep_first=keep_first, keep_last=keep_last, kv_lens=kv_lens,
                                **_select_kwargs(rule_param, rule)).contiguous()


@attn_sparge_select_kvlen.register_fake
def _(q, k, v, simthreshd1, rule_param, rule, keep_first, keep_last, kv_lens, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape)


@torch.library.custom_op("sageattention_amd::attn_sparge_select_lse_kvlen", mutates_args=())
def attn_sparge_select_lse_kvlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, simthreshd1: torch.Tensor,
                                 rule_param: torch.Tensor, rule: str, keep_first: int, keep_last: int, kv_lens: torch.Tensor,
                                 tensor_layout: str, sm_scale: float, pv: str,
                                 qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    o, lse = core.sageattn_sparge(q, k, v, tensor_layout=tensor_layout, simthreshd1=simthreshd1, sm_scale=sm_scale, pv=pv,
                                  qk_quant_gran=qk_quant_gran, return_lse=True, keep_first=keep_first, keep_last=keep_last,
                                  kv_lens=kv_lens, **_select_kwargs(rule_param, rule))
    return o.contiguous(), lse


@attn_sparge_select_lse_kvlen.register_fake
def _(q, k, v, simthreshd1, rule_param, rule, keep_first, keep_last, kv_lens, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _lse_like(q, tensor_layout)


@torch.library.custom_op("sageattention_amd::attn_sparge_pv_kvlen", mutates_args=())
def attn_sparge_pv_kvlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, simthreshd1: torch.Tensor, rule_param: torch.Tensor,
                         rule: str, keep_first: int, keep_last: int, pvthreshd: torch.Tensor, kv_lens: torch.Tensor,
                         tensor_layout: str, sm_scale: float, pv: str, qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    o, skipped = core.sageattn_sparge(q, k, v, tensor_layout=tensor_layout, simthreshd1=simthreshd1, sm_scale=sm_scale, pv=pv,
                                      qk_quant_gran=qk_quant_gran, keep_first=keep_first, keep_last=keep_last,
                                      pvthreshd=pvthreshd, return_skipped=True, kv_lens=kv_lens,
                                      **_select_kwargs(rule_param, rule))
    return o.contiguous(), skipped


@attn_sparge_pv_kvlen.register_fake
def _(q, k, v, simthreshd1, rule_param, rule, keep_first, keep_last, pvthreshd, kv_lens, tensor_layout, sm_scale, pv,
      qk_quant_gran):
    return q.new_empty(q.shape), _skipped_like(q, tensor_layout)


@torch.library.custom_op("sageattention_amd::attn_sparge_pv_lse_kvlen", mutates_args=())
def attn_sparge_pv_lse_kvlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, simthreshd1: torch.Tensor,
                             rule_param: torch.Tensor, rule: str, keep_first: int, keep_last: int, pvthreshd: torch.Tensor,
                             kv_lens: torch.Tensor, tensor_layout: str, sm_scale: float, pv: str,
                             qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    o, lse, skipped = core.sageattn_sparge(q, k, v, tensor_layout=tensor_layout, simthreshd1=simthreshd1, sm_scale=sm_scale,
                                           pv=pv, qk_quant_gran=qk_quant_gran, return_lse=True, keep_first=keep_first,
                                           keep_last=keep_last, pvthreshd=pvthreshd, return_skipped=True, kv_lens=kv_lens,
                                           **_select_kwargs(rule_param, rule))
    return o.contiguous(), lse, skipped


@attn_sparge_pv_lse_kvlen.register_fake
def _(q, k, v, simthreshd1, rule_param, rule, keep_first, keep_last, pvthreshd, kv_lens, tensor_layout, sm_scale, pv,
      qk_quant_gran):
    return q.new_empty(q.shape), _lse_like(q, tensor_layout), _skipped_like(q, tensor_layout)


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
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")
    core._check_select_args(topk, keep_first, keep_last)
    core._check_pvskip_args(pvthreshd, return_skipped)
    if sm_scale is None:
        sm_scale = q.size(-1) ** -0.5
    rule, par = ("cdf", cdfthreshd) if topk is None else ("topk", topk)
    thr, par = _as_per_head(simthreshd1, q, tensor_layout), _as_per_head(par, q, tensor_layout)
    ns = torch.ops.sageattention_amd
    if kv_lens is not None:
        tail = (kv_lens, tensor_layout, float(sm_scale), pv, qk_quant_gran)
        if pvthreshd is not None:
            pvt = _as_per_head(pvthreshd, q, tensor_layout)
            op = ns.attn_sparge_pv_lse_kvlen if return_lse else ns.attn_sparge_pv_kvlen
            out = op(q, k, v, thr, par, rule, keep_first, keep_last, pvt, *tail)
            out = out if return_skipped else out[:-1]
            return out if len(out) > 1 else out[0]
        op = ns.attn_sparge_select_lse_kvlen if return_lse else ns.attn_sparge_select_kvlen
        return op(q, k, v, thr, par, rule, keep_first, keep_last, *tail)
    if pvthreshd is not None:
        pvt = _as_per_head(pvthreshd, q, tensor_layout)
        op = torch.ops.sageattention_amd.attn_sparge_pv_lse if return_lse else torch.ops.sageattention_amd.attn_sparge_pv
        out = op(q, k, v, thr, par, rule, keep_first, keep_last, pvt, tensor_layout, float(sm_scale), pv, qk_quant_gran)
        out = out if return_skipped else out[:-1]
        return out if len(out) > 1 else out[0]
    if topk is None and keep_first == 0 and keep_last == 0:
        op = torch.ops.sageattention_amd.attn_sparge_lse if return_lse else torch.ops.sageattention_amd.attn_sparge
        return op(q, k, v, thr, par, tensor_layout, float(sm_scale), pv, qk_quant_gran)
    op = torch.ops.sageattention_amd.attn_sparge_select_lse if return_lse else torch.ops.sageattention_amd.attn_sparge_select
    return op(q, k, v, thr, par, rule, keep_first, keep_last, tensor_layout, float(sm_scale), pv, qk_quant_gran)


@torch.library.custom_op("sageattention_amd::attn_kvlen", mutates_args=())
def attn_kvlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_lens: torch.Tensor, tensor_layout: str, is_causal: bool,
               sm_scale: float, pv: str, qk_quant_gran: str) -> torch.Tensor:
    return core.sageattn_kvlen(q, k, v, kv_lens, tensor_layout=tensor_layout, is_causal=is_causal, sm_scale=sm_scale, pv=pv,
                               qk_quant_gran=qk_quant_gran).contiguous()


@attn_kvlen.register_fake
def _(q, k, v, kv_lens, tensor_layout, is_causal, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape)


@torch.library.custom_op("sageattention_amd::attn_kvlen_lse", mutates_args=())
def attn_kvlen_lse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_lens: torch.Tensor, tensor_layout: str,
                   is_causal: bool, sm_scale: float, pv: str, qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    o, lse = core.sageattn_kvlen(q, k, v, kv_lens, tensor_layout=tensor_layout, is_causal=is_causal, sm_scale=sm_scale, pv=pv,
                                 qk_quant_gran=qk_quant_gran, return_lse=True)
    return o.contiguous(), lse


@attn_kvlen_lse.register_fake
def _(q, k, v, kv_lens, tensor_layout, is_causal, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _lse_like(q, tensor_layout)


def sageattn_kvlen_compilable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_lens: torch.Tensor,
                              tensor_layout: str = "HND", is_causal: bool = False, sm_scale: Optional[float] = None,
                              pv: str = "fp16", qk_quant_gran: str = "per_thread", return_lse: bool = False):
    """``sageattn_kvlen`` (core.py) as a traceable custom op: ``kv_lens`` is the int32 [B] tensor of valid keys per batch."""
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")
    if sm_scale is None:
        sm_scale = q.size(-1) ** -0.5
    op = torch.ops.sageattention_amd.attn_kvlen_lse if return_lse else torch.ops.sageattention_amd.attn_kvlen
    return op(q, k, v, kv_lens, tensor_layout, bool(is_causal), float(sm_scale), pv, qk_quant_gran)


@torch.library.custom_op("sageattention_amd::attn_splitkv", mutates_args=())
def attn_splitkv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_lens: Optional[torch.Tensor], num_splits: int,
                 tensor_layout: str, sm_scale: float, pv: str, qk_quant_gran: str) -> torch.Tensor:
    return core.sageattn_splitkv(q, k, v, kv_lens=kv_lens, num_splits=num_splits or None, tensor_layout=tensor_layout,
                                 sm_scale=sm_scale, pv=pv, qk_quant_gran=qk_quant_gran).contiguous()


@attn_splitkv.register_fake
def _(q, k, v, kv_lens, num_splits, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape)


@torch.library.custom_op("sageattention_amd::attn_splitkv_lse", mutates_args=())
def attn_splitkv_lse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_lens: Optional[torch.Tensor], num_splits: int,
                     tensor_layout: str, sm_scale: float, pv: str, qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    o, lse = core.sageattn_splitkv(q, k, v, kv_lens=kv_lens, num_splits=num_splits or None, tensor_layout=tensor_layout,
                                   sm_scale=sm_scale, pv=pv, qk_quant_gran=qk_quant_gran, return_lse=True)
    return o.contiguous(), lse


@attn_splitkv_lse.register_fake
def _(q, k, v, kv_lens, num_splits, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _lse_like(q, tensor_layout)


def _splitkv_compilable_args(q, tensor_layout, num_splits, sm_scale):
    """what the two split-KV wrappers below check, and the op's forms of num_splits (0: automatic) and sm_scale"""
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")
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
    op = torch.ops.sageattention_amd.attn_splitkv_lse if return_lse else torch.ops.sageattention_amd.attn_splitkv
    return op(q, k, v, kv_lens, num_splits, tensor_layout, sm_scale, pv, qk_quant_gran)


@torch.library.custom_op("sageattention_amd::attn_splitkv_causal", mutates_args=())
def attn_splitkv_causal(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_lens: Optional[torch.Tensor], num_splits: int,
                        q_fold: int, tensor_layout: str, sm_scale: float, pv: str, qk_quant_gran: str) -> torch.Tensor:
    return core.sageattn_splitkv_causal(q, k, v, kv_lens=kv_lens, num_splits=num_splits or None, q_fold=q_fold,
                                        tensor_layout=tensor_layout, sm_scale=sm_scale, pv=pv,
                                        qk_quant_gran=qk_quant_gran).contiguous()


@attn_splitkv_causal.register_fake
def _(q, k, v, kv_lens, num_splits, q_fold, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape)


@torch.library.custom_op("sageattention_amd::attn_splitkv_causal_lse", mutates_args=())
def attn_splitkv_causal_lse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_lens: Optional[torch.Tensor],
                            num_splits: int, q_fold: int, tensor_layout: str, sm_scale: float, pv: str,
                            qk_quant_gran: str) -> Tuple[torch.Tensor, torch.Tensor]:
    o, lse = core.sageattn_splitkv_causal(q, k, v, kv_lens=kv_lens, num_splits=num_splits or None, q_fold=q_fold,
                                          tensor_layout=tensor_layout, sm_scale=sm_scale, pv=pv, qk_quant_gran=qk_quant_gran,
                                          return_lse=True)
    return o.contiguous(), lse


@attn_splitkv_causal_lse.register_fake
def _(q, k, v, kv_lens, num_splits, q_fold, tensor_layout, sm_scale, pv, qk_quant_gran):
    return q.new_empty(q.shape), _lse_like(q, tensor_layout)


def sageattn_splitkv_causal_compilable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                       kv_lens: Optional[torch.Tensor] = None, num_splits: Optional[int] = None,
                                       q_fold: int = 1, tensor_layout: str = "HND", sm_scale: Optional[float] = None,
                                       pv: str = "fp16", qk_quant_gran: str = "per_thread", return_lse: bool = False):
    """``sageattn_splitkv_causal`` (core.py) as a traceable custom op: ``kv_lens`` is an optional int32 [B] tensor argument of
    the op, ``num_splits`` an int with 0 for the automatic choice (``core.splitkv_num_splits``), ``q_fold`` the query rows per
    token."""
    num_splits, sm_scale = _splitkv_compilable_args(q, tensor_layout, num_splits, sm_scale)
    ns = torch.ops.sageattention_amd
    op = ns.attn_splitkv_causal_lse if return_lse else ns.attn_splitkv_causal
    return op(q, k, v, kv_lens, num_splits, q_fold, tensor_layout, sm_scale, pv, qk_quant_gran)


def sageattn_compilable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tensor_layout: str = "HND",
                        is_causal: bool = False, sm_scale: Optional[float] = None, return_lse: bool = False,
                        pv: str = "auto", qk_quant_gran: str = "per_thread", **kwargs: Any):
    """``sageattn`` (core.py:80-144) as a traceable custom op.  ``pv="auto"`` follows the dispatcher of the package
    (``core.dispatch_pv``: FP8 PV from a few thousand keys per row upwards, FP16 PV below; per_thread scales); unknown
    keyword arguments are accepted and ignored like there."""
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")
    if pv == "auto":
        pv = core.dispatch_pv(q, k, tensor_layout, bool(is_causal))
    if sm_scale is None:
        sm_scale = q.size(-1) ** -0.5
    if return_lse:
        return torch.ops.sageattention_amd.attn_lse(q, k, v, tensor_layout, bool(is_causal), float(sm_scale), pv,
                                                    qk_quant_gran)
    return torch.ops.sageattention_amd.attn(q, k, v, tensor_layout, bool(is_causal), float(sm_scale), pv, qk_quant_gran)
