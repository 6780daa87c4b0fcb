"""Sliding-window attention and sink logits on the paged quantized KV cache (include/sageattn_hip_window.h holds the rule).

Mistral and Gemma 2/3 attend only the last ``window`` keys in most layers; gpt-oss does so in every other layer and adds a
learned per-head *sink* logit to every softmax denominator.  ``sageattn_splitkv_paged_window`` and
``sageattn_splitkv_paged_ragged_window`` are ``sageattn_splitkv_paged(causal=True)`` and ``sageattn_splitkv_paged_ragged`` with
those two additions: row r (token t = r / g) attends exactly the keys ``max(0, t + off_b - window + 1) <= j <= t + off_b``,
``off_b = len_b - T_b``.  A q-block's tile range starts at the tile of its first row's lower limit, so a decode step reads
``window`` rows of K and V instead of ``len_b``, and no block-table entry below ``max(off_b - window + 1, 0) // page_size`` is
used to form an address: an engine may free the pages that have left the window.

The sink logit is in the units of the returned LSE (natural log of the scaled logits) and belongs to the query head -- in a
folded row ``t * g + i`` of KV head hk that is head ``hk * g + i``.  It is applied once, in the merge, after the ``q . km``
correction: ``lse' = logaddexp(lse, sink_h)``, ``o' = o * exp(lse - lse')``, one rounding to the output dtype.

With ``window >= len_b`` and ``num_splits=1`` (or one q-block per sequence, any ``num_splits``) and no sinks, o and lse have the
bits of the parent operators.  The ops live in ``torch.ops.sageattention_amd_window``: ``attn_splitkv_paged_window[_lse]`` and
``attn_splitkv_paged_ragged_window[_lse]``; they trace under ``torch.compile(fullgraph=True)`` and capture into a HIP graph.

Not built: the contiguous caches, the FP4 paged cache, the shared-prefix operator, a non-causal or dense windowed form, sink
*tokens* (StreamingLLM's pinned first keys) and a ``window`` that differs per sequence."""
from typing import Any, Optional

import torch

from . import _lib as L
from . import core
from . import paged
from . import ragged
from .paged_fp4 import SagePagedKVCacheV4

__all__ = ["sageattn_splitkv_paged_window", "sageattn_splitkv_paged_ragged_window"]

_NS = "sageattention_amd_window"


# ---- ops ----------------------------------------------------------------------------------------------------------------------
def _attn_body(is_ragged, with_lse):
    def body(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, *rest):
        cu_seqlens_q, items = rest[:2] if is_ragged else (None, None)
        num_splits, q_fold, window, sinks, tensor_layout, sm_scale, qk_quant_gran = rest[-7:]
        P, Hk, page_size, _ = L.dims(k8, tensor_layout)
        lib = L.lib()
        pv_fp8 = v_scale is not None
        want_lse = with_lse or sinks is not None  # (the merge needs the corrected LSE of every row for the sink term)
        with torch.cuda.device(q.device):
            q = core._abi_view(q)  # (a view the C ABI cannot address travels as a contiguous copy, as in the operators)
            o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
            if is_ragged:
                M, Hq, D = q.shape
                B = block_table.size(0)
                lse_shape, ws_bytes = (M, Hq), lib.sage_ragged_workspace_bytes(M, Hq, D, num_splits)
                qd, od = (L.SageTensor(t.data_ptr(), 0, t.stride(1), t.stride(0)) for t in (q, o))
                mid = (kv_lens.data_ptr(), cu_seqlens_q.data_ptr(), items.data_ptr(), items.size(0), int(num_splits), int(q_fold))
            else:
                B, Hq, M, D = L.dims(q, tensor_layout)
                lse_shape, ws_bytes = (B, Hq, M), lib.sage_splitkv_workspace_bytes(B, Hq, M, D, num_splits)
                qd, od = L.desc(q, tensor_layout), L.desc(o, tensor_layout)
                mid = (kv_lens.data_ptr(), int(num_splits), 1, int(q_fold))
            lse = torch.empty(lse_shape, dtype=torch.float32, device=q.device) if want_lse else None
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
            fn = f"sage_attn_fusedq_pv_{'f8' if pv_fp8 else 'f16'}_splitkv_paged_{'ragged_' * is_ragged}window"
            # in the order of the C signatures: the f8 form has no v_dtype and takes v_scale
            v_args = (L.desc_vt(v, tensor_layout),) if pv_fp8 else (L.desc(v, tensor_layout), L.dtype_code(v.dtype))
            L.check(getattr(lib, fn)(
                qd, L.dtype_code(q.dtype), L.desc(k8, tensor_layout), *v_args, od, L.dtype_code(o.dtype), k_scale.data_ptr(),
                km.data_ptr(), *((v_scale.data_ptr(),) if pv_fp8 else ()), L.ptr(lse), B, Hq, Hk, M, D,
                core._GRAN_CODE[qk_quant_gran], 32, float(sm_scale), *paged._table_args(block_table, page_size, P), *mid,
                ws.data_ptr(), ws.numel(), L.stream_ptr(q.device), min(int(window), 2 ** 31 - 1), L.ptr(sinks)), fn)
        return (o, lse) if with_lse else o

    def fake(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, *rest):
        o = q.new_empty(q.shape)
        if not with_lse:
            return o
        return o, q.new_empty(q.shape[:2] if is_ragged else L.dims(q, rest[-3])[:3], dtype=torch.float32)

    return body, fake


_HEAD = "Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor block_table, Tensor kv_lens, "
_TAIL = ("SymInt num_splits, SymInt q_fold, SymInt window, Tensor? sinks, str tensor_layout, float sm_scale, "
         "str qk_quant_gran")
for _ragged in (False, True):
    for _lse in (False, True):
        _name = f"attn_splitkv_paged_{'ragged_' * _ragged}window{'_lse' * _lse}"
        _schema = f"({_HEAD}{'Tensor cu_seqlens_q, Tensor items, ' * _ragged}{_TAIL}) -> {'(Tensor, Tensor)' if _lse else 'Tensor'}"
        _body, _fake = _attn_body(_ragged, _lse)
        torch.library.custom_op(f"{_NS}::{_name}", _body, mutates_args=(), schema=_schema).register_fake(_fake)


# ---- the public interface ------------------------------------------------------------------------------------------------------
def _check_window(window, sinks, Hq, device):
    """what the window operators refuse by name beyond their parents: ``window`` and ``sinks``"""
    if isinstance(window, bool) or not isinstance(window, int):
        raise TypeError(f"window must be an int >= 1, got {type(window).__name__}")
    if window < 1:
        raise ValueError(f"window must be >= 1, got {window}")
    if sinks is None:
        return None
    if not isinstance(sinks, torch.Tensor):
        raise TypeError("sinks must be a float32 tensor of shape [Hq] or None")
    if sinks.dtype != torch.float32:
        raise TypeError(f"sinks must be of dtype float32, got {sinks.dtype}")
    if tuple(sinks.shape) != (Hq,):
        raise ValueError(f"sinks shape {tuple(sinks.shape)} does not match [Hq] = [{Hq}]")
    if sinks.device != device:
        raise ValueError(f"sinks is on {sinks.device}, q on {device}")
    return sinks.contiguous()


def _check_cache(cache):
    if isinstance(cache, SagePagedKVCacheV4):
        raise TypeError("cache must be a SagePagedKVCache or a SagePagedRowCache, got SagePagedKVCacheV4: a sliding window on "
                        "the FP4 paged cache is not built")
    if not isinstance(cache, tuple(paged._CACHE_TYPES)):
        raise TypeError(f"cache must be a SagePagedKVCache or a SagePagedRowCache, got {type(cache).__name__}")


def _windowed_keys(block_table, cache, window, q_fold):
    """the most keys a q-block walks: what ``splitkv_num_splits`` sees in the place of N"""
    return min(block_table.size(1) * cache.page_size, window + 128 // q_fold)


def sageattn_splitkv_paged_window(q: torch.Tensor, cache, block_table: torch.Tensor, kv_lens: torch.Tensor, window: int,
                                  num_splits: Optional[int] = None, q_fold: int = 1, sinks: Optional[torch.Tensor] = None,
                                  sm_scale: Optional[float] = None, return_lse: bool = False, **refused: Any):
    """``sageattn_splitkv_paged(causal=True)`` with a sliding window and optional sink logits: arguments, layouts, ``cache``
    (``SagePagedKVCache`` or ``SagePagedRowCache``; P.V fp16, bf16 or fp8) and ``q_fold`` are the parent's.  Row r of the
    ``M / q_fold`` tokens attends the keys ``max(0, t + off_b - window + 1) <= j <= t + off_b``; a row with ``t + off_b < 0`` and
    every row of a sequence without keys gives o = 0, lse = -inf, with or without sinks.

    ``window``: a Python int >= 1, one per call.  ``sinks``: fp32, one value per UN-folded query head (``q.size(1) * q_fold``
    of them, the model's Hq), on q's device, or None.  ``num_splits``: 1..16, or None for ``splitkv_num_splits`` on
    ``min(max_pages * page_size, window + 128 // q_fold)`` keys in the place of N -- a guess that nobody has measured.  Refused
    by name, before any launch: ``window < 1``, ``sinks`` of another shape, dtype or device, the FP4 paged cache, and what the
    parent refuses."""
    _check_cache(cache)
    block_table = paged._check_block_table(block_table, q.size(0), cache.device)
    k_like = cache.k if isinstance(cache, paged.SagePagedKVCache) else cache.k8
    if kv_lens is None:
        raise TypeError("kv_lens must be an int32 tensor of shape [B]")
    kv_lens, ns, M = core._splitkv_front("sageattn_splitkv_causal", True, q, k_like, k_like, kv_lens, num_splits,
                                         cache.tensor_layout, cache.pv, cache.qk_quant_gran, refused)
    ragged._check_fold(q_fold)
    if M % q_fold != 0:
        raise ValueError(f"q_fold must be >= 1 and divide the {M} query rows, got {q_fold}")
    if q.dtype != cache.dtype or q.device != cache.device:
        raise ValueError("q must have the dtype and device of the cache's k")
    D = cache.head_dim
    if q.size(-1) != D:
        raise ValueError(f"q must have the cache's head_dim {D}, got {q.size(-1)}")
    B, Hq = L.dims(q, cache.tensor_layout)[:2]
    if Hq % cache.num_kv_heads != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({cache.num_kv_heads})")
    if cache.km.size(0) != B:
        raise ValueError(f"q has {B} sequences, the cache {cache.km.size(0)}")
    sinks = _check_window(window, sinks, Hq * q_fold, q.device)
    if num_splits is None:  # (the existing rule on the windowed key count: not measured)
        ns = core.splitkv_num_splits(B, Hq, M, _windowed_keys(block_table, cache, window, q_fold))
    fp8 = cache.pv == "fp8"
    op = getattr(getattr(torch.ops, _NS), f"attn_splitkv_paged_window{'_lse' if return_lse else ''}")
    return op(q, cache.k8, cache.k_scale, cache.km, cache.v8 if fp8 else cache.v, cache.v_scale if fp8 else None, block_table,
              kv_lens, ns, q_fold, window, sinks, cache.tensor_layout, float(D ** -0.5 if sm_scale is None else sm_scale),
              cache.qk_quant_gran)


def sageattn_splitkv_paged_ragged_window(q: torch.Tensor, cache, block_table: torch.Tensor, kv_lens: torch.Tensor,
                                         cu_seqlens_q: torch.Tensor, window: int, plan: Optional[ragged.RaggedQPlan] = None,
                                         num_splits: Optional[int] = None, q_fold: int = 1,
                                         sinks: Optional[torch.Tensor] = None, sm_scale: Optional[float] = None,
                                         return_lse: bool = False, **refused: Any):
    """``sageattn_splitkv_paged_ragged`` with a sliding window and optional sink logits; ``plan`` is the parent's
    ``ragged_q_plan``, unchanged.  For each sequence the rows have the bits of ``sageattn_splitkv_paged_window`` on that
    sequence alone.  ``sinks``: fp32, one value per un-folded query head (``[Hq]``), or None.  ``num_splits``: 1..16, or None for ``splitkv_num_splits(1, Hq // g,
    128 * n_items, min(max_pages * page_size, window + 128 // g))`` -- a guess that nobody has measured.  Refusals as
    ``sageattn_splitkv_paged_window`` and the parent."""
    _check_cache(cache)
    if not isinstance(q, torch.Tensor) or q.dim() != 3 or q.size(0) < 1:
        raise ValueError("q must be a [total_tokens >= 1, Hq, D] tensor")
    if q.stride(-1) != 1:
        raise ValueError("q must have a contiguous last dim (stride(-1) == 1)")
    if kv_lens is None:
        raise TypeError("kv_lens must be an int32 tensor of shape [B]")
    core._splitkv_front("sageattn_splitkv_causal", True, q.unsqueeze(0), cache.k8, cache.k8, None, num_splits,
                        cache.tensor_layout, cache.pv, cache.qk_quant_gran, refused)
    cu_seqlens_q = ragged._check_cu(cu_seqlens_q)
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
    ragged._check_fold(q_fold)
    if q_fold not in (1, Hq // Hk):
        raise ValueError(f"q_fold must be 1 or Hq / Hk = {Hq // Hk}, got {q_fold}")
    if cache.km.size(0) != B:
        raise ValueError(f"cu_seqlens_q has {B} sequences, the cache {cache.km.size(0)}")
    sinks = _check_window(window, sinks, Hq, q.device)
    if plan is None:
        items = torch.ops.sageattention_amd_ragged.ragged_q_plan(cu_seqlens_q, T, q_fold)
    elif not isinstance(plan, ragged.RaggedQPlan):
        raise TypeError(f"plan must be a RaggedQPlan or None, got {type(plan).__name__}")
    elif (plan.B, plan.total_tokens, plan.q_fold) != (B, T, q_fold):
        raise ValueError(f"plan was made for (B, total_tokens, q_fold) = {(plan.B, plan.total_tokens, plan.q_fold)}, the call "
                         f"has {(B, T, q_fold)}")
    else:
        items = plan.items
    if num_splits is None:  # (the existing rule on the list's size and the windowed key count: not measured)
        num_splits = core.splitkv_num_splits(1, Hq // q_fold, 128 * ragged._n_items(B, T, q_fold),
                                             _windowed_keys(block_table, cache, window, q_fold))
    fp8 = cache.pv == "fp8"
    op = getattr(getattr(torch.ops, _NS), f"attn_splitkv_paged_ragged_window{'_lse' if return_lse else ''}")
    return op(q, cache.k8, cache.k_scale, cache.km, cache.v8 if fp8 else cache.v, cache.v_scale if fp8 else None, block_table,
              kv_lens, cu_seqlens_q, items, num_splits, q_fold, window, sinks, cache.tensor_layout,
              float(D ** -0.5 if sm_scale is None else sm_scale), cache.qk_quant_gran)
