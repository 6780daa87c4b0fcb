"""Decode attention on the paged MXFP4 V cache: one wave per split (include/sageattn_hip_decode_fp4.h holds the rule).

``SagePagedKVCacheV4`` is the cache with the fewest bytes per key -- at head_dim 128 128 B of INT8 K, 64 B of e2m1 V and 4 scale
bytes -- and was the one cache ``sageattn_decode_paged`` (decode.py) could not serve: its decode steps ran the four-wave
``sageattn_splitkv_paged_v4(causal=True)``, three waves of which work for rows nobody stores.  ``sageattn_decode_paged_v4`` runs
``attn_i8_decode_paged_v4_kernel`` (``csrc/sage_attn_decode.hip``): the one-wave kernel of decode.py whose V never touches LDS.
In the image the MFMA fragment of a lane is 16 contiguous bytes of the pool, and a one-wave workgroup has no other wave that
wants them, so every lane loads its ``D / 32`` fragments and its scale word a tile ahead, straight into registers; the LDS ring
holds K alone.

The operator is always bottom-right causal -- row r is token ``t = r // q_fold`` and attends the keys ``0 <= j <= t + len_b - T``
-- and o and lse are **bit-identical** to ``sageattn_splitkv_paged_v4(q, cache, block_table, kv_lens, num_splits=S, causal=True,
q_fold=g)`` for every S, length and page size.  Nothing dispatches to it implicitly.

Ops: ``torch.ops.sageattention_amd_decode_fp4.attn_decode_paged_v4[_lse]``; they trace under ``torch.compile(fullgraph=True)``
and capture into a HIP graph whose replay follows a table and lengths rewritten in place.

Not built: the contiguous ``SageKVCacheV4``, the ragged, window, sink and shared-prefix forms, an FP4 image for
``SagePagedRowCache``, more than 16 splits, more than 32 rows, a merge inside the attention launch, and FP4 for P, Q or K."""
from typing import Any, Optional

import torch

from . import _lib as L
from . import core
from .decode import DECODE_MAX_ROWS, decode_num_splits
from .paged import _check_block_table, _table_args
from .paged_fp4 import SagePagedKVCacheV4, _img_desc

__all__ = ["sageattn_decode_paged_v4", "sageattn_decode_paged_v4_compilable"]

_NS = "sageattention_amd_decode_fp4"


# ---- ops ----------------------------------------------------------------------------------------------------------------------
def _attn_body(with_lse):
    def body(q, k8, k_scale, km, v4, v4_scale, block_table, kv_lens, num_splits, q_fold, tensor_layout, sm_scale, qk_quant_gran):
        B, Hq, M, D = L.dims(q, tensor_layout)
        P, Hk, page_size, _ = L.dims(k8, tensor_layout)
        num_splits = num_splits or decode_num_splits(B, Hq, block_table.size(1) * page_size)
        lib = L.lib()
        with torch.cuda.device(q.device):
            q = core._abi_view(q)  # (a view the C ABI cannot address travels as a contiguous copy, as in the operators)
            o = torch.empty(q.size(), dtype=q.dtype, device=q.device)
            lse = torch.empty((B, Hq, M), dtype=torch.float32, device=q.device) if with_lse else None
            ws = torch.empty(lib.sage_splitkv_workspace_bytes(B, Hq, M, D, num_splits), dtype=torch.uint8, device=q.device)
            L.check(lib.sage_attn_fusedq_pv_f4_decode_paged(
                L.desc(q, tensor_layout), L.dtype_code(q.dtype), L.desc(k8, tensor_layout), _img_desc(v4), L.desc(o, tensor_layout),
                L.dtype_code(o.dtype), k_scale.data_ptr(), km.data_ptr(), v4_scale.data_ptr(), L.ptr(lse), B, Hq, Hk, M, D,
                core._GRAN_CODE[qk_quant_gran], 32, float(sm_scale), *_table_args(block_table, page_size, P), kv_lens.data_ptr(),
                int(num_splits), int(q_fold), ws.data_ptr(), ws.numel(), L.stream_ptr(q.device)),
                "sage_attn_fusedq_pv_f4_decode_paged")
        return (o, lse) if with_lse else o

    def fake(q, k8, k_scale, km, v4, v4_scale, block_table, kv_lens, num_splits, q_fold, tensor_layout, sm_scale, qk_quant_gran):
        o = q.new_empty(q.shape)
        return (o, q.new_empty(L.dims(q, tensor_layout)[:3], dtype=torch.float32)) if with_lse else o

    return body, fake


_SCHEMA = ("(Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v4, Tensor v4_scale, Tensor block_table, Tensor kv_lens, "
           "SymInt num_splits, SymInt q_fold, str tensor_layout, float sm_scale, str qk_quant_gran)")
for _lse in (False, True):
    _body, _fake = _attn_body(_lse)
    torch.library.custom_op(f"{_NS}::attn_decode_paged_v4{'_lse' * _lse}", _body, mutates_args=(),
                            schema=f"{_SCHEMA} -> {'(Tensor, Tensor)' if _lse else 'Tensor'}").register_fake(_fake)


def _call(q, cache, block_table, kv_lens, num_splits, q_fold, sm_scale, return_lse):
    kc = cache._kc
    op = getattr(getattr(torch.ops, _NS), f"attn_decode_paged_v4{'_lse' if return_lse else ''}")
    return op(q, kc.k8, kc.k_scale, kc.km, cache.v4, cache.v4_scale, block_table, kv_lens, num_splits, q_fold, kc.tensor_layout,
              float(kc.head_dim ** -0.5 if sm_scale is None else sm_scale), kc.qk_quant_gran)


# ---- the public interface ------------------------------------------------------------------------------------------------------
def sageattn_decode_paged_v4_compilable(q: torch.Tensor, cache: SagePagedKVCacheV4, block_table: torch.Tensor,
                                        kv_lens: torch.Tensor, num_splits: int = 0, q_fold: int = 1,
                                        sm_scale: Optional[float] = None, return_lse: bool = False):
    """``sageattn_decode_paged_v4`` as a traceable custom-op call on the pools of ``cache``: no argument checks of its own beyond
    the op's; ``num_splits`` 0 means ``decode_num_splits``."""
    return _call(q, cache, block_table, kv_lens, num_splits, q_fold, sm_scale, return_lse)


def sageattn_decode_paged_v4(q: torch.Tensor, cache: SagePagedKVCacheV4, block_table: torch.Tensor, kv_lens: torch.Tensor,
                             num_splits: Optional[int] = None, q_fold: int = 1, sm_scale: Optional[float] = None,
                             return_lse: bool = False, **refused: Any):
    """Decode attention on a ``SagePagedKVCacheV4`` (head_dim 64 or 128): the one-wave attention launch over (sequence, head,
    split) and the merge of ``sageattn_splitkv_paged_v4``.

    ``q`` is ``[B, Hk, R, D]`` (NHD: ``[B, R, Hk, D]``), already folded by the caller exactly as for
    ``sageattn_splitkv_paged_v4(causal=True, q_fold=g)``: ``R = T * g <= 32`` rows are T tokens, the last positions of the
    sequence's ``len_b`` keys, and row r attends the keys ``0 <= j <= r // g + len_b - T``.  A row without a key and a
    sequence without keys give o = 0, lse = -inf; rows at or beyond ``len_b``, table entries at or beyond
    ``ceil(len_b / page_size)`` and pages the sequence does not name influence nothing.  o and lse have the bits of
    ``sageattn_splitkv_paged_v4(..., num_splits=S, causal=True, q_fold=g)`` for every S.

    ``num_splits``: 1..16, or None for ``decode_num_splits(B, Hk, max_pages * page_size)``.  ``R > 32`` raises a ValueError
    that names ``sageattn_splitkv_paged_v4``; what that operator refuses is refused here in the same words."""
    if not isinstance(cache, SagePagedKVCacheV4):
        raise TypeError(f"cache must be a SagePagedKVCacheV4, got {type(cache).__name__}")
    kc = cache._kc
    block_table = _check_block_table(block_table, q.size(0), kc.device)
    if kv_lens is None:
        raise TypeError("kv_lens must be an int32 tensor of shape [B]")
    kv_lens, ns, M = core._splitkv_front("sageattn_splitkv_causal", True, q, kc.k, kc.v, kv_lens, num_splits, kc.tensor_layout,
                                         "fp8", kc.qk_quant_gran, refused)
    if isinstance(q_fold, bool) or not isinstance(q_fold, int):
        raise TypeError(f"q_fold must be an int >= 1, got {type(q_fold).__name__}")
    if q_fold < 1 or M % q_fold != 0:
        raise ValueError(f"q_fold must be >= 1 and divide the {M} query rows (and 1 unless causal), got {q_fold}")
    if q.dtype != kc.dtype or q.device != kc.device:
        raise ValueError("q must have the dtype and device of the cache's k")
    D = kc.head_dim
    if q.size(-1) != D:
        raise ValueError(f"q must have the cache's head_dim {D}, got {q.size(-1)}")
    B, Hq = L.dims(q, kc.tensor_layout)[:2]
    if Hq % kc.num_kv_heads != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({kc.num_kv_heads})")
    if kc.km.size(0) != B:
        raise ValueError(f"q has {B} sequences, the cache {kc.km.size(0)}")
    if M > DECODE_MAX_ROWS:
        raise ValueError(f"sageattn_decode_paged_v4 takes at most {DECODE_MAX_ROWS} query rows (tokens * q_fold), got {M}: use "
                         "sageattn_splitkv_paged_v4(causal=True)")
    if num_splits is None:  # (from the logical capacity: the pool's third dim is one page)
        ns = decode_num_splits(B, Hq, block_table.size(1) * kc.page_size)
    return _call(q, cache, block_table, kv_lens, ns, q_fold, sm_scale, return_lse)
