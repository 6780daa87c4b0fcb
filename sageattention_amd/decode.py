"""Decode attention on the paged quantized KV cache: one wave per split (include/sageattn_hip_decode.h holds the rule).

``sageattn_splitkv_paged`` attends 128 query rows per workgroup with four waves of 32 rows each.  A decode step folded by its GQA
group has 4 to 32 rows: three of the four waves then read every K and V fragment, issue every MFMA and take every exponential
for rows nobody stores, and the step's time follows that loop and not the bytes of the cache.  ``sageattn_decode_paged`` runs a
kernel shaped for at most 32 query rows (``csrc/sage_attn_decode.hip``): a workgroup is ONE wave and one split of one
(sequence, head), with a private LDS ring it fills itself by LDS-DMA and orders with counted ``vmcnt`` waits alone.

The operator is always bottom-right causal -- row r is token ``t = r // q_fold`` and attends the keys ``0 <= j <= t + len_b - T``
-- and o and lse are **bit-identical** to ``sageattn_splitkv_paged(q, cache, block_table, kv_lens, num_splits=S, causal=True,
q_fold=g)`` for every S, length and page size: the split ranges, the workspace and the merge are that operator's, and the kernel
does the arithmetic of that kernel's first wave in that wave's order.  Nothing dispatches to it implicitly.

Ops: ``torch.ops.sageattention_amd_decode.attn_decode_paged[_lse]``; they trace under ``torch.compile(fullgraph=True)`` and
capture into a HIP graph whose replay follows a table and lengths rewritten in place.

The paged MXFP4 V cache has an operator of its own, ``sageattn_decode_paged_v4`` (decode_fp4.py).

A sliding window, sink logits and -- with one split -- the merge inside the attention launch: ``sageattn_decode_paged_window``
(decode_window.py).

Not built: the contiguous caches, the ragged and shared-prefix forms, more than 16 splits, more than 32 rows, and a merge inside
the attention launch of this operator."""
from typing import Any, Optional

import torch

from . import _lib as L
from . import core
from . import paged

__all__ = ["sageattn_decode_paged", "sageattn_decode_paged_compilable", "decode_num_splits"]

_NS = "sageattention_amd_decode"

DECODE_MAX_ROWS = 32        # one wave: one 32-row block of query rows
DECODE_MIN_TILES = 4        # key tiles (of 64) a split should keep
DECODE_SLOTS = 3 * 256      # resident one-wave workgroups of an MI355X at head_dim 128 with 16-bit P.V: three per CU, 256 CUs


def decode_num_splits(B: int, Hk: int, capacity_keys: int) -> int:
    """The number of splits ``sageattn_decode_paged(num_splits=None)`` takes: from the shape alone (no host synchronisation;
    ``kv_lens`` does not enter),

        min(16, ceil(ntk / 4), floor(3 * 256 / (B * Hk))), at least 1,      ntk = ceil(capacity_keys / 64),

    ``Hk`` the heads of the folded q.  The third term takes the most splits with which the grid ``B * Hk * S`` still fits the
    768 one-wave workgroups an MI355X holds at once with the largest ring (three per CU: head_dim 128, 16-bit P.V) -- rounded
    DOWN: a grid that just overshoots the resident slots runs a second, mostly empty round (measured: 64 * 8 * 2 = 1024
    workgroups took 331 us where S = 1 took 301 us, and S = 13 at B = 8 steps up from 49 to 62 us).  The second term keeps at
    least 4 key tiles per split, so that the ring fills once and runs; the first is the merge kernel's slot count.  The two
    constants are a GUESS from the kernel's geometry for 16-bit P.V at head_dim 128 and were not tuned per P.V type or head
    dim.  Against the sweep of ``tools/decode_bench.py`` over S in 1..16 (profiles/decode.md) the rule's choice is the best S
    or within 1 % of it with FP8 P.V and at B = 64, 3.1-3.3 % off at (8, 32, 1, 8192, 128) and 3.9-4.3 % off for 4 speculative
    tokens with FP16 P.V (S = 8 is best there, the rule takes 12); one long sequence wants more than 16 splits, which is not built."""
    ntk = (int(capacity_keys) + 63) // 64
    grid = max(int(B) * int(Hk), 1)
    return max(1, min(core.SPLITKV_MAX, -(-ntk // DECODE_MIN_TILES), DECODE_SLOTS // grid))


# ---- ops ----------------------------------------------------------------------------------------------------------------------
def _attn_body(with_lse):
    def body(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, num_splits, q_fold, tensor_layout, sm_scale, qk_quant_gran):
        B, Hq, M, D = L.dims(q, tensor_layout)
        P, Hk, page_size, _ = L.dims(k8, tensor_layout)
        num_splits = num_splits or decode_num_splits(B, Hq, block_table.size(1) * page_size)
        lib = L.lib()
        pv_fp8 = v_scale is not None
        with torch.cuda.device(q.device):
            q = core._abi_view(q)  # (a view the C ABI cannot address travels as a contiguous copy, as in the operators)
            o = torch.empty(q.size(), dtype=q.dtype, device=q.device)
            lse = torch.empty((B, Hq, M), dtype=torch.float32, device=q.device) if with_lse else None
            ws = torch.empty(lib.sage_splitkv_workspace_bytes(B, Hq, M, D, num_splits), dtype=torch.uint8, device=q.device)
            fn = f"sage_attn_fusedq_pv_{'f8' if pv_fp8 else 'f16'}_decode_paged"
            # in the order of the C signatures: the f8 form has no v_dtype and takes v_scale
            v_args = (L.desc_vt(v, tensor_layout),) if pv_fp8 else (L.desc(v, tensor_layout), L.dtype_code(v.dtype))
            L.check(getattr(lib, fn)(
                L.desc(q, tensor_layout), L.dtype_code(q.dtype), L.desc(k8, tensor_layout), *v_args, L.desc(o, tensor_layout),
                L.dtype_code(o.dtype), k_scale.data_ptr(), km.data_ptr(), *((v_scale.data_ptr(),) if pv_fp8 else ()), L.ptr(lse),
                B, Hq, Hk, M, D, core._GRAN_CODE[qk_quant_gran], 32, float(sm_scale),
                *paged._table_args(block_table, page_size, P), kv_lens.data_ptr(), int(num_splits), int(q_fold), ws.data_ptr(),
                ws.numel(), L.stream_ptr(q.device)), fn)
        return (o, lse) if with_lse else o

    def fake(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, num_splits, q_fold, tensor_layout, sm_scale, qk_quant_gran):
        o = q.new_empty(q.shape)
        return (o, q.new_empty(L.dims(q, tensor_layout)[:3], dtype=torch.float32)) if with_lse else o

    return body, fake


_SCHEMA = ("(Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor block_table, Tensor kv_lens, "
           "SymInt num_splits, SymInt q_fold, str tensor_layout, float sm_scale, str qk_quant_gran)")
for _lse in (False, True):
    _body, _fake = _attn_body(_lse)
    torch.library.custom_op(f"{_NS}::attn_decode_paged{'_lse' * _lse}", _body, mutates_args=(),
                            schema=f"{_SCHEMA} -> {'(Tensor, Tensor)' if _lse else 'Tensor'}").register_fake(_fake)


# ---- the public interface ------------------------------------------------------------------------------------------------------
def sageattn_decode_paged_compilable(q: torch.Tensor, cache, block_table: torch.Tensor, kv_lens: torch.Tensor,
                                     num_splits: int = 0, q_fold: int = 1, sm_scale: Optional[float] = None,
                                     return_lse: bool = False):
    """``sageattn_decode_paged`` as a traceable custom-op call on the pools of ``cache``: no argument checks of its own beyond
    the op's; ``num_splits`` 0 means ``decode_num_splits``."""
    fp8 = cache.pv == "fp8"
    op = getattr(getattr(torch.ops, _NS), f"attn_decode_paged{'_lse' if return_lse else ''}")
    return op(q, cache.k8, cache.k_scale, cache.km, cache.v8 if fp8 else cache.v, cache.v_scale if fp8 else None, block_table,
              kv_lens, num_splits, q_fold, cache.tensor_layout, float(cache.head_dim ** -0.5 if sm_scale is None else sm_scale),
              cache.qk_quant_gran)


def sageattn_decode_paged(q: torch.Tensor, cache, block_table: torch.Tensor, kv_lens: torch.Tensor,
                          num_splits: Optional[int] = None, q_fold: int = 1, sm_scale: Optional[float] = None,
                          return_lse: bool = False, **refused: Any):
    """Decode attention on a ``SagePagedKVCache`` or a ``SagePagedRowCache`` (P.V fp16, bf16 or fp8; head_dim 64 or 128): the
    one-wave attention launch over (sequence, head, split) and the merge of ``sageattn_splitkv_paged``.

    ``q`` is ``[B, Hk, R, D]`` (NHD: ``[B, R, Hk, D]``), already folded by the caller exactly as for
    ``sageattn_splitkv_paged(causal=True, q_fold=g)``: ``R = T * g <= 32`` rows are T tokens, the last positions of the
    sequence's ``len_b`` keys, and row r attends the keys ``0 <= j <= r // g + len_b - T``.  A row without a key and a
    sequence without keys give o = 0, lse = -inf; rows at or beyond ``len_b`` of the last page and table entries at or beyond
    ``ceil(len_b / page_size)`` influence nothing.  o and lse have the bits of ``sageattn_splitkv_paged(..., num_splits=S,
    causal=True, q_fold=g)`` for every S.

    ``num_splits``: 1..16, or None for ``decode_num_splits(B, Hk, max_pages * page_size)``.  ``R > 32`` raises a ValueError
    that names ``sageattn_splitkv_paged``; what that operator refuses is refused here in the same words."""
    if not isinstance(cache, tuple(paged._CACHE_TYPES)):
        raise TypeError(f"cache must be a SagePagedKVCache, got {type(cache).__name__}")
    block_table, kv_lens, ns, M = paged._attn_front(q, cache, block_table, kv_lens, num_splits, True, q_fold, refused)
    if M > DECODE_MAX_ROWS:
        raise ValueError(f"sageattn_decode_paged takes at most {DECODE_MAX_ROWS} query rows (tokens * q_fold), got {M}: use "
                         "sageattn_splitkv_paged(causal=True)")
    D = cache.head_dim
    B, Hq = L.dims(q, cache.tensor_layout)[:2]
    if num_splits is None:  # (from the logical capacity: the pool's third dim is one page)
        ns = decode_num_splits(B, Hq, block_table.size(1) * cache.page_size)
    fp8 = cache.pv == "fp8"
    op = getattr(getattr(torch.ops, _NS), f"attn_decode_paged{'_lse' if return_lse else ''}")
    return op(q, cache.k8, cache.k_scale, cache.km, cache.v8 if fp8 else cache.v, cache.v_scale if fp8 else None, block_table,
              kv_lens, ns, q_fold, cache.tensor_layout, float(D ** -0.5 if sm_scale is None else sm_scale), cache.qk_quant_gran)
