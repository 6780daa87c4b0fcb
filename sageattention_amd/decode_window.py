"""Decode attention with a sliding window and sink logits on the paged quantized KV cache: one wave per split, and with one
split ONE launch (include/sageattn_hip_decode_window.h holds the rule).

gpt-oss has a sink logit in every layer and a 128-key window in every other one; Mistral and Gemma 2/3 attend a window only.
``sageattn_decode_paged`` is always full-causal and has no sinks, so their decode steps went through the four-wave kernels of
``sageattn_splitkv_paged_window``, where three of the four waves work for rows nobody stores.  ``sageattn_decode_paged_window``
runs the one-wave kernel (``csrc/sage_attn_decode_window.hip``) with a two-sided limit: row r (token ``t = r // q_fold``)
attends exactly the keys ``max(0, t + off_b - window + 1) <= j <= t + off_b``, ``off_b = len_b - T``, a step reads ``window``
rows of K and V instead of ``len_b``, and no block-table entry below ``max(off_b - window + 1, 0) // page_size`` is used to form
an address.

With one split -- a 128-key window is two or three tiles -- the merge launch would only add ``q . km``, apply the sink and round.
The kernel does that in its epilogue instead: the step is one launch, and the op allocates no workspace.  With more splits the
partials go through the merge of ``sageattn_splitkv_paged_window``.  Either way o and lse are **bit-identical** to
``sageattn_splitkv_paged_window(q, cache, block_table, kv_lens, window, num_splits=S, q_fold=g, sinks=sinks)`` for every S,
window, length and page size; with ``window`` at or beyond the capacity and no sinks they have the bits of
``sageattn_decode_paged``.  Nothing dispatches to the operator implicitly.

Ops: ``torch.ops.sageattention_amd_decode_window.attn_decode_paged_window[_lse]``; they trace under
``torch.compile(fullgraph=True)`` and capture into a HIP graph whose replay follows a table and lengths rewritten in place.

Not built: the FP4 paged cache, the ragged and shared-prefix decode forms, a finish inside the launch for more than one split or
in ``sageattn_decode_paged``, more than 16 splits, more than 32 rows, and a ``window`` that differs per sequence."""
from typing import Any, Optional

import torch

from . import _lib as L
from . import core
from . import paged
from . import window as W
from .decode import DECODE_MAX_ROWS, decode_num_splits

__all__ = ["sageattn_decode_paged_window", "sageattn_decode_paged_window_compilable"]

_NS = "sageattention_amd_decode_window"


def _num_splits(B, Hk, capacity_keys, window, q_fold, M):
    """``decode_num_splits`` on the keys a windowed step walks, ``min(capacity, window + 64 + T)``: the window, the tokens of the
    step and the tile the range starts inside"""
    return decode_num_splits(B, Hk, min(int(capacity_keys), int(window) + 64 + M // max(int(q_fold), 1)))


# ---- ops ----------------------------------------------------------------------------------------------------------------------
def _attn_body(with_lse):
    def body(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, num_splits, q_fold, window, sinks, tensor_layout, sm_scale,
             qk_quant_gran):
        B, Hq, M, D = L.dims(q, tensor_layout)
        P, Hk, page_size, _ = L.dims(k8, tensor_layout)
        num_splits = num_splits or _num_splits(B, Hq, block_table.size(1) * page_size, window, q_fold, M)
        lib = L.lib()
        pv_fp8 = v_scale is not None
        want_lse = with_lse or sinks is not None  # (the sink term needs the corrected LSE of every row)
        with torch.cuda.device(q.device):
            q = core._abi_view(q)  # (a view the C ABI cannot address travels as a contiguous copy, as in the operators)
            o = torch.empty(q.size(), dtype=q.dtype, device=q.device)
            lse = torch.empty((B, Hq, M), dtype=torch.float32, device=q.device) if want_lse else None
            ws = None  # one split: the kernel finishes the rows itself, there is no workspace
            if num_splits != 1:
                ws = torch.empty(lib.sage_splitkv_workspace_bytes(B, Hq, M, D, num_splits), dtype=torch.uint8, device=q.device)
            fn = f"sage_attn_fusedq_pv_{'f8' if pv_fp8 else 'f16'}_decode_paged_window"
            # in the order of the C signatures: the f8 form has no v_dtype and takes v_scale
            v_args = (L.desc_vt(v, tensor_layout),) if pv_fp8 else (L.desc(v, tensor_layout), L.dtype_code(v.dtype))
            L.check(getattr(lib, fn)(
                L.desc(q, tensor_layout), L.dtype_code(q.dtype), L.desc(k8, tensor_layout), *v_args, L.desc(o, tensor_layout),
                L.dtype_code(o.dtype), k_scale.data_ptr(), km.data_ptr(), *((v_scale.data_ptr(),) if pv_fp8 else ()), L.ptr(lse),
                B, Hq, Hk, M, D, core._GRAN_CODE[qk_quant_gran], 32, float(sm_scale),
                *paged._table_args(block_table, page_size, P), kv_lens.data_ptr(), int(num_splits), int(q_fold), L.ptr(ws),
                0 if ws is None else ws.numel(), L.stream_ptr(q.device), min(int(window), 2 ** 31 - 1), L.ptr(sinks)), fn)
        return (o, lse) if with_lse else o

    def fake(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, num_splits, q_fold, window, sinks, tensor_layout, sm_scale,
             qk_quant_gran):
        o = q.new_empty(q.shape)
        return (o, q.new_empty(L.dims(q, tensor_layout)[:3], dtype=torch.float32)) if with_lse else o

    return body, fake


_SCHEMA = ("(Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor block_table, Tensor kv_lens, "
           "SymInt num_splits, SymInt q_fold, SymInt window, Tensor? sinks, str tensor_layout, float sm_scale, "
           "str qk_quant_gran)")
for _lse in (False, True):
    _body, _fake = _attn_body(_lse)
    torch.library.custom_op(f"{_NS}::attn_decode_paged_window{'_lse' * _lse}", _body, mutates_args=(),
                            schema=f"{_SCHEMA} -> {'(Tensor, Tensor)' if _lse else 'Tensor'}").register_fake(_fake)


# ---- the public interface ------------------------------------------------------------------------------------------------------
def _call(q, cache, block_table, kv_lens, window, num_splits, q_fold, sinks, sm_scale, return_lse):
    fp8 = cache.pv == "fp8"
    op = getattr(getattr(torch.ops, _NS), f"attn_decode_paged_window{'_lse' if return_lse else ''}")
    return op(q, cache.k8, cache.k_scale, cache.km, cache.v8 if fp8 else cache.v, cache.v_scale if fp8 else None, block_table,
              kv_lens, num_splits, q_fold, window, sinks, cache.tensor_layout,
              float(cache.head_dim ** -0.5 if sm_scale is None else sm_scale), cache.qk_quant_gran)


def sageattn_decode_paged_window_compilable(q: torch.Tensor, cache, block_table: torch.Tensor, kv_lens: torch.Tensor,
                                            window: int, num_splits: int = 0, q_fold: int = 1,
                                            sinks: Optional[torch.Tensor] = None, sm_scale: Optional[float] = None,
                                            return_lse: bool = False):
    """``sageattn_decode_paged_window`` as a traceable custom-op call on the pools of ``cache``: no argument checks of its own
    beyond the op's; ``num_splits`` 0 means the rule of ``sageattn_decode_paged_window``."""
    return _call(q, cache, block_table, kv_lens, window, num_splits, q_fold, sinks, sm_scale, return_lse)


def sageattn_decode_paged_window(q: torch.Tensor, cache, block_table: torch.Tensor, kv_lens: torch.Tensor, window: int,
                                 num_splits: Optional[int] = None, q_fold: int = 1, sinks: Optional[torch.Tensor] = None,
                                 sm_scale: Optional[float] = None, return_lse: bool = False, **refused: Any):
    """Decode attention with a sliding window and optional sink logits on a ``SagePagedKVCache`` or a ``SagePagedRowCache``
    (P.V fp16, bf16 or fp8; head_dim 64 or 128; pages of 64, 128 or 256 keys).

    ``q`` is ``[B, Hk, R, D]`` (NHD: ``[B, R, Hk, D]``), folded as for ``sageattn_decode_paged``: ``R = T * g <= 32`` rows are
    T tokens, the last positions of the sequence's ``len_b`` keys, and row r attends the keys ``max(0, t + off_b - window + 1)
    <= j <= t + off_b`` with ``t = r // g`` and ``off_b = len_b - T``.  A row without a key and a sequence without keys give
    o = 0, lse = -inf, with or without sinks.  ``window``: a Python int >= 1, one per call.  ``sinks``: fp32, one value per
    UN-folded query head (``q.size(1) * q_fold`` of them, the model's Hq), on q's device, or None; it is applied once, behind
    the ``q . km`` correction.  o and lse have the bits of ``sageattn_splitkv_paged_window(..., num_splits=S, q_fold=g,
    sinks=sinks)`` for every S.

    ``num_splits``: 1..16, or None for ``decode_num_splits(B, Hk, min(max_pages * page_size, window + 64 + T))`` -- a GUESS
    that nobody has measured.  With one split the call is ONE launch and takes no workspace; with more it is the attention
    launch and the merge of ``sageattn_splitkv_paged_window``.  ``R > 32`` raises a ValueError that names
    ``sageattn_splitkv_paged_window``; ``window``, ``sinks`` and the FP4 paged cache are refused in that operator's words, the
    rest in those of ``sageattn_splitkv_paged``."""
    W._check_cache(cache)
    block_table, kv_lens, ns, M = paged._attn_front(q, cache, block_table, kv_lens, num_splits, True, q_fold, refused)
    if M > DECODE_MAX_ROWS:
        raise ValueError(f"sageattn_decode_paged_window takes at most {DECODE_MAX_ROWS} query rows (tokens * q_fold), got {M}: "
                         "use sageattn_splitkv_paged_window")
    B, Hq = L.dims(q, cache.tensor_layout)[:2]
    sinks = W._check_window(window, sinks, Hq * q_fold, q.device)
    if num_splits is None:  # (the decode rule on the windowed key count: not measured)
        ns = _num_splits(B, Hq, block_table.size(1) * cache.page_size, window, q_fold, M)
    return _call(q, cache, block_table, kv_lens, window, ns, q_fold, sinks, sm_scale, return_lse)
