"""Ragged-query attention on the paged quantized KV cache: one call per layer for a MIXED batch (include/sageattn_hip_ragged.h
holds the rule).

A serving engine with continuous batching holds a prefill chunk of 2048 tokens beside 63 decode sequences of one token each,
the queries packed as ``[total_tokens, Hq, D]`` with a ``cu_seqlens_q``.  ``sageattn_splitkv_paged`` takes one M for the whole
batch, so such a step pads every sequence to the longest chunk or makes one call per chunk length, and either way copies q to
fold the GQA group into rows.  Here sequence b has its own ``T_b = cu[b+1] - cu[b]`` tokens, the LAST positions of its
``len_b`` keys; a small planning kernel turns ``cu_seqlens_q`` into a work list of the 128-row q-blocks that exist, the
attention grid is that list x heads x splits, and the kernel reads q and writes o in the engine's own layout: the fold costs
nothing.  Every sequence's rows are bit-identical to ``sageattn_splitkv_paged(causal=True)`` on that sequence alone.

Everything is read on the device only, so {plan; attention} captures into one HIP graph.  The ops live in a namespace of their
own, ``torch.ops.sageattention_amd_ragged``: ``ragged_q_plan`` and ``attn_splitkv_paged_ragged[_lse]``; they trace under
``torch.compile(fullgraph=True)``.

Not built: ragged queries on the FP4 paged cache (``SagePagedKVCacheV4``) and on the contiguous caches, a non-causal ragged
form, packed new rows for ``SagePagedRowCache.append_rows`` (it still takes ``[B, Hk, T, D]``; ``SagePagedKVCache.append``
already serves ragged growth through ``start_lens`` / ``kv_lens``), a split count per sequence, ordering the work list by
cost, and the shared-prefix operator with ragged suffix queries."""
from typing import Any, Optional

import torch

from . import _lib as L
from . import core
from . import paged
from .paged_fp4 import SagePagedKVCacheV4

__all__ = ["RaggedQPlan", "ragged_q_plan", "sageattn_splitkv_paged_ragged"]

_NS = "sageattention_amd_ragged"


def _n_items(B, total_tokens, q_fold):
    """slots of the work list: an upper bound of sum_b ceil(T_b * g / 128) that shapes alone give"""
    return total_tokens * q_fold // 128 + B


# ---- ops ----------------------------------------------------------------------------------------------------------------------
def _plan_body(cu_seqlens_q, total_tokens, q_fold):
    B = cu_seqlens_q.numel() - 1
    items = torch.empty((_n_items(B, total_tokens, q_fold), 2), dtype=torch.int32, device=cu_seqlens_q.device)
    with torch.cuda.device(cu_seqlens_q.device):
        L.check(L.lib().sage_ragged_q_plan(cu_seqlens_q.data_ptr(), B, int(total_tokens), int(q_fold), items.data_ptr(),
                                           items.size(0), L.stream_ptr(cu_seqlens_q.device)), "sage_ragged_q_plan")
    return items


def _plan_fake(cu_seqlens_q, total_tokens, q_fold):
    return cu_seqlens_q.new_empty((_n_items(cu_seqlens_q.numel() - 1, total_tokens, q_fold), 2))


def _attn_body(with_lse):
    def body(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, cu_seqlens_q, items, num_splits, q_fold, tensor_layout,
             sm_scale, qk_quant_gran):
        T, Hq, D = q.shape
        P, Hk, page_size, _ = L.dims(k8, tensor_layout)
        B = block_table.size(0)
        lib = L.lib()
        pv_fp8 = v_scale is not None
        with torch.cuda.device(q.device):
            q = core._abi_view(q)  # (a view the C ABI cannot address travels as a contiguous copy, as in the operators)
            o = torch.empty((T, Hq, D), dtype=q.dtype, device=q.device)
            lse = torch.empty((T, Hq), dtype=torch.float32, device=q.device) if with_lse else None
            ws = torch.empty(lib.sage_ragged_workspace_bytes(T, Hq, D, num_splits), dtype=torch.uint8, device=q.device)
            fn = f"sage_attn_fusedq_pv_{'f8' if pv_fp8 else 'f16'}_splitkv_paged_ragged"
            # q and o as [B,H,N,D] descriptors whose N is the token: stride_b is not read
            qd, od = (L.SageTensor(t.data_ptr(), 0, t.stride(1), t.stride(0)) for t in (q, o))
            # in the order of the C signatures: the f8 form has no v_dtype and takes v_scale
            v_args = (L.desc_vt(v, tensor_layout),) if pv_fp8 else (L.desc(v, tensor_layout), L.dtype_code(v.dtype))
            L.check(getattr(lib, fn)(
                qd, L.dtype_code(q.dtype), L.desc(k8, tensor_layout), *v_args, od, L.dtype_code(o.dtype), k_scale.data_ptr(),
                km.data_ptr(), *((v_scale.data_ptr(),) if pv_fp8 else ()), L.ptr(lse), B, Hq, Hk, T, D,
                core._GRAN_CODE[qk_quant_gran], 32, float(sm_scale), *paged._table_args(block_table, page_size, P),
                kv_lens.data_ptr(), cu_seqlens_q.data_ptr(), items.data_ptr(), items.size(0), int(num_splits), int(q_fold),
                ws.data_ptr(), ws.numel(), L.stream_ptr(q.device)), fn)
        return (o, lse) if with_lse else o

    def fake(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, cu_seqlens_q, items, num_splits, q_fold, tensor_layout,
             sm_scale, qk_quant_gran):
        o = q.new_empty(q.shape)
        return (o, q.new_empty(q.shape[:2], dtype=torch.float32)) if with_lse else o

    return body, fake


# name, schema, body, fake: one row per op of the namespace
_ATTN_PARAMS = ("Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor block_table, Tensor kv_lens, "
                "Tensor cu_seqlens_q, Tensor items, SymInt num_splits, SymInt q_fold, str tensor_layout, float sm_scale, "
                "str qk_quant_gran")
_OPS = (
    ("ragged_q_plan", "(Tensor cu_seqlens_q, SymInt total_tokens, SymInt q_fold) -> Tensor", _plan_body, _plan_fake),
    ("attn_splitkv_paged_ragged", f"({_ATTN_PARAMS}) -> Tensor", *_attn_body(False)),
    ("attn_splitkv_paged_ragged_lse", f"({_ATTN_PARAMS}) -> (Tensor, Tensor)", *_attn_body(True)),
)
for _name, _schema, _body, _fake in _OPS:
    torch.library.custom_op(f"{_NS}::{_name}", _body, mutates_args=(), schema=_schema).register_fake(_fake)


# ---- the public interface ------------------------------------------------------------------------------------------------------
class RaggedQPlan:
    """The work list of a step (``ragged_q_plan``): int32 ``[n_items, 2]`` pairs (sequence, 128-row q-block) on the device,
    b = -1 in unused slots, and the shapes it was made for.  It depends on ``cu_seqlens_q``, ``total_tokens`` and ``q_fold``
    only: one plan serves every layer of a step."""
    __slots__ = ("items", "B", "total_tokens", "q_fold")

    def __init__(self, items, B, total_tokens, q_fold):
        self.items, self.B, self.total_tokens, self.q_fold = items, B, total_tokens, q_fold


def _check_cu(cu_seqlens_q):
    """``cu_seqlens_q`` as the kernels read it: int32 [B + 1], B >= 1, contiguous (its values stay on the device)"""
    if not isinstance(cu_seqlens_q, torch.Tensor):
        raise TypeError("cu_seqlens_q must be an int32 tensor of shape [B + 1]")
    if cu_seqlens_q.dtype != torch.int32:
        raise TypeError(f"cu_seqlens_q must be of dtype int32, got {cu_seqlens_q.dtype}")
    if cu_seqlens_q.dim() != 1 or cu_seqlens_q.size(0) < 2:
        raise ValueError(f"cu_seqlens_q shape {tuple(cu_seqlens_q.shape)} does not match [B + 1], B >= 1")
    return cu_seqlens_q.contiguous()


def _check_fold(q_fold):
    if isinstance(q_fold, bool) or not isinstance(q_fold, int):
        raise TypeError(f"q_fold must be an int >= 1, got {type(q_fold).__name__}")
    if q_fold < 1:
        raise ValueError(f"q_fold must be >= 1, got {q_fold}")


def ragged_q_plan(cu_seqlens_q: torch.Tensor, total_tokens: int, q_fold: int = 1) -> RaggedQPlan:
    """The work list of ``sageattn_splitkv_paged_ragged`` for these query lengths: one launch of one workgroup, which scans
    ``ceil(T_b * q_fold / 128)`` over the sequences and writes one pair per q-block that exists, in sequence order, into
    ``total_tokens * q_fold // 128 + B`` slots.  Deterministic; ``cu_seqlens_q`` is read on the device only.  Stated and not
    checked: ``cu[0] = 0``, non-decreasing, ``cu[B] = total_tokens``."""
    cu_seqlens_q = _check_cu(cu_seqlens_q)
    if isinstance(total_tokens, bool) or not isinstance(total_tokens, int):
        raise TypeError(f"total_tokens must be an int >= 1, got {type(total_tokens).__name__}")
    if total_tokens < 1:
        raise ValueError(f"total_tokens must be >= 1, got {total_tokens}")
    _check_fold(q_fold)
    items = getattr(torch.ops, _NS).ragged_q_plan(cu_seqlens_q, total_tokens, q_fold)
    return RaggedQPlan(items, cu_seqlens_q.size(0) - 1, total_tokens, q_fold)


def sageattn_splitkv_paged_ragged(q: torch.Tensor, cache, block_table: torch.Tensor, kv_lens: torch.Tensor,
                                  cu_seqlens_q: torch.Tensor, plan: Optional[RaggedQPlan] = None,
                                  num_splits: Optional[int] = None, q_fold: int = 1, sm_scale: Optional[float] = None,
                                  return_lse: bool = False, **refused: Any):
    """Causal split-KV attention of packed queries on a ``SagePagedKVCache`` or ``SagePagedRowCache``.  ``q`` is
    ``[total_tokens, Hq, D]`` with ``stride(-1) == 1`` and any token and head strides (a view into a fused QKV projection
    output is read in place); sequence b owns the tokens ``[cu[b], cu[b+1])`` of it, and token t of its ``T_b`` attends the
    keys ``j <= t + len_b - T_b``, ``len_b = clamp(kv_lens[b], 0, max_pages * page_size)``: the tokens are the last positions
    of the sequence's keys.  A token whose bound is negative, and every token of a sequence without keys, gives o = 0 and
    lse = -inf; a sequence without tokens writes nothing and nothing of its table row is read.  Returns o
    ``[total_tokens, Hq, D]`` contiguous in q's dtype, and with ``return_lse`` the natural-log lse fp32 ``[total_tokens, Hq]``.

    ``q_fold`` = g is 1 or ``Hq / Hk``.  With ``Hq / Hk`` the g query heads of a KV head become query rows, token-major, as in
    ``sageattn_splitkv_causal``: row ``t * g + i`` of KV head hk is ``q[token t, head hk * g + i]``.  The kernel's addressing
    does the fold; nothing is copied.  For every sequence the rows of its tokens are bit-identical to
    ``sageattn_splitkv_paged(q_b, cache.narrow(b, 1), block_table[b:b+1], kv_lens[b:b+1], num_splits, causal=True, q_fold=g)``
    with ``q_b`` folded by hand into ``[1, Hq / g, T_b * g, D]``.

    ``plan``: the ``ragged_q_plan`` of ``(cu_seqlens_q, total_tokens, q_fold)``, or None to build it inside the call.
    ``num_splits``: 1..16 for the whole call, or None for ``splitkv_num_splits(1, Hq // g, 128 * n_items, max_pages *
    page_size)``, the existing rule on the work list's size -- a guess that nobody has measured on a mixed batch.  There is no
    ``causal`` keyword.  Stated and not checked: ``cu[0] = 0``, non-decreasing, ``cu[B] = total_tokens``; a ``cu_seqlens_q``
    that breaks them gives undefined values but no access outside the buffers.  What ``sageattn_splitkv_paged`` refuses by
    name is refused here in the same words."""
    if isinstance(cache, SagePagedKVCacheV4):
        raise TypeError("cache must be a SagePagedKVCache or a SagePagedRowCache, got SagePagedKVCacheV4: ragged queries on the "
                        "FP4 paged cache are not built")
    if not isinstance(cache, tuple(paged._CACHE_TYPES)):
        raise TypeError(f"cache must be a SagePagedKVCache or a SagePagedRowCache, got {type(cache).__name__}")
    if not isinstance(q, torch.Tensor) or q.dim() != 3 or q.size(0) < 1:
        raise ValueError("q must be a [total_tokens >= 1, Hq, D] tensor")
    if q.stride(-1) != 1:
        raise ValueError("q must have a contiguous last dim (stride(-1) == 1)")
    if kv_lens is None:
        raise TypeError("kv_lens must be an int32 tensor of shape [B]")
    # the refused keywords, the strings and num_splits, in the words of sageattn_splitkv_paged(causal=True)
    core._splitkv_front("sageattn_splitkv_causal", True, q.unsqueeze(0), cache.k8, cache.k8, None, num_splits,
                        cache.tensor_layout, cache.pv, cache.qk_quant_gran, refused)
    cu_seqlens_q = _check_cu(cu_seqlens_q)
    B = cu_seqlens_q.size(0) - 1
    block_table = paged._check_block_table(block_table, B, cache.device)
    kv_lens = core._check_kv_lens(kv_lens, B, q.device)
    if cu_seqlens_q.device != q.device:
        raise ValueError(f"cu_seqlens_q is on {cu_seqlens_q.device}, q on {q.device}")
    if q.dtype != cache.dtype or q.device != cache.device:
        raise ValueError("q must have the dtype and device of the cache's k")
    T, Hq, D = q.shape
    if D != cache.head_dim:
        raise ValueError(f"q must have the cache's head_dim {cache.head_dim}, got {D}")
    Hk = cache.num_kv_heads
    if Hq % Hk != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({Hk})")
    _check_fold(q_fold)
    if q_fold not in (1, Hq // Hk):
        raise ValueError(f"q_fold must be 1 or Hq / Hk = {Hq // Hk}, got {q_fold}")
    if cache.km.size(0) != B:
        raise ValueError(f"cu_seqlens_q has {B} sequences, the cache {cache.km.size(0)}")
    ops = getattr(torch.ops, _NS)
    if plan is None:
        items = ops.ragged_q_plan(cu_seqlens_q, T, q_fold)
    elif not isinstance(plan, RaggedQPlan):
        raise TypeError(f"plan must be a RaggedQPlan or None, got {type(plan).__name__}")
    elif (plan.B, plan.total_tokens, plan.q_fold) != (B, T, q_fold):
        raise ValueError(f"plan was made for (B, total_tokens, q_fold) = {(plan.B, plan.total_tokens, plan.q_fold)}, the call "
                         f"has {(B, T, q_fold)}")
    else:
        items = plan.items
    if num_splits is None:  # (the existing rule on the list's size: not measured on a mixed batch)
        num_splits = core.splitkv_num_splits(1, Hq // q_fold, 128 * _n_items(B, T, q_fold), block_table.size(1) * cache.page_size)
    if sm_scale is None:
        sm_scale = D ** -0.5
    fp8 = cache.pv == "fp8"
    op = getattr(ops, f"attn_splitkv_paged_ragged{'_lse' if return_lse else ''}")
    return op(q, cache.k8, cache.k_scale, cache.km, cache.v8 if fp8 else cache.v, cache.v_scale if fp8 else None, block_table,
              kv_lens, cu_seqlens_q, items, num_splits, q_fold, cache.tensor_layout, float(sm_scale), cache.qk_quant_gran)
