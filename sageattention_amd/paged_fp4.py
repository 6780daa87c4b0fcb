"""The MXFP4 V image of ``SageKVCacheV4`` (fp4.py) for a KV cache kept in pages: ``SagePagedKVCache`` (paged.py) with V as
FP4 nibbles and e8m0 scale bytes per page (include/sageattn_hip_paged_fp4.h holds the rule).

A scale group of the image lies inside one 64-key tile, like the scale groups of K, and nothing of V is frozen, so a page's
image bytes depend on the page's own rows only: paging is an addressing change.  Every valid tile of the paged state and
every o / lse of ``sageattn_splitkv_paged_v4`` is bit-identical to ``SageKVCacheV4`` / ``sageattn_splitkv_v4`` on the padded
tensors gathered from the pages, and lse to the paged FP8 cache's on the same K.

    cache = SagePagedKVCacheV4.prepare(k_pool, v_pool, block_table, kv_lens)    bind the pools, freeze km, write the pages
    cache.append(block_table, start_lens, kv_lens, max_new)                       ONE launch: K and the image
    o = sageattn_splitkv_paged_v4(q, cache, block_table, kv_lens)                 no gather: the attention launch and the merge

The block table is passed on every call and is not stored; it and the lengths are read on the device only, so
{append; attention} captures into one HIP graph.  The ops live in ``torch.ops.sageattention_amd_paged_fp4``:
``kv_cache_append_paged_v4`` (it mutates the state pools) and ``attn_splitkv[_causal]_paged_v4[_lse]``; everything traces
under ``torch.compile(fullgraph=True)``.

Not built: an FP4 image for ``SagePagedRowCache`` (a scale group is a maximum over 32 tokens: it would need an fp16 V tail
per sequence); the shared-prefix operator on this cache; page sizes below 64; FP4 for P, Q or K."""
from typing import Any, Optional

import torch

from . import _lib as L
from . import core
from .paged import SagePagedKVCache, _check_block_table, _table_args

__all__ = ["SagePagedKVCacheV4", "sageattn_splitkv_paged_v4"]

_NS = "sageattention_amd_paged_fp4"


def _img_desc(img):
    """the pool of images [P,Hk,D,32*tpp]: stride_b the stride of a page, stride_n that of a channel"""
    return L.SageTensor(img.data_ptr(), img.stride(0), img.stride(1), img.stride(2))


# ---- ops ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::kv_cache_append_paged_v4", mutates_args=("k8", "k_scale", "v4", "v4_scale"))
def kv_cache_append_paged_v4(k: torch.Tensor, v: torch.Tensor, km: torch.Tensor, k8: torch.Tensor, k_scale: torch.Tensor,
                             v4: torch.Tensor, v4_scale: torch.Tensor, block_table: torch.Tensor, start_lens: torch.Tensor,
                             kv_lens: torch.Tensor, max_new: int, tensor_layout: str, qk_quant_gran: str) -> None:
    """sage_kv_cache_append_paged_v4 on the pools of a cache: one launch for K and the image"""
    P, H, page_size, D = L.dims(k, tensor_layout)
    gran, rnd = core._k_pairing(qk_quant_gran)
    with torch.cuda.device(k.device):
        L.check(L.lib().sage_kv_cache_append_paged_v4(
            L.desc(k, tensor_layout), L.desc(v, tensor_layout), L.dtype_code(k.dtype), block_table.size(0), H, D, km.data_ptr(),
            L.desc(k8, tensor_layout), k_scale.data_ptr(), gran, rnd, _img_desc(v4), v4_scale.data_ptr(),
            *_table_args(block_table, page_size, P), start_lens.data_ptr(), kv_lens.data_ptr(), int(max_new),
            L.stream_ptr(k.device)), "sage_kv_cache_append_paged_v4")


@kv_cache_append_paged_v4.register_fake
def _(k, v, km, k8, k_scale, v4, v4_scale, block_table, start_lens, kv_lens, max_new, tensor_layout, qk_quant_gran):
    return None


def _register_attn(name, causal, with_lse):
    """attn_splitkv[_causal]_paged_v4[_lse]: sage_attn_fusedq_pv_f4_splitkv_paged on the pools of a cache -- the workspace, the
    attention launch over the splits and the merge; num_splits 0 = ``core.splitkv_num_splits`` on the logical capacity; o is
    contiguous in q's shape"""
    params = ("Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v4, Tensor v4_scale, Tensor block_table, Tensor kv_lens, "
              "SymInt num_splits, " + "SymInt q_fold, " * causal + "str tensor_layout, float sm_scale, str qk_quant_gran")

    def body(q, k8, k_scale, km, v4, v4_scale, block_table, kv_lens, num_splits, *rest):
        q_fold = rest[0] if causal else 1
        tensor_layout, sm_scale, qk_quant_gran = rest[-3:]
        B, Hq, M, D = L.dims(q, tensor_layout)
        P, Hk, page_size, _ = L.dims(k8, tensor_layout)
        num_splits = num_splits or core.splitkv_num_splits(B, Hq, M, block_table.size(1) * page_size)
        lib = L.lib()
        with torch.cuda.device(q.device):
            q = core._abi_view(q)  # (a view the C ABI cannot address travels as a contiguous copy, as in the operators)
            o = torch.empty(q.size(), dtype=q.dtype, device=q.device)
            lse = torch.empty((B, Hq, M), dtype=torch.float32, device=q.device) if with_lse else None
            ws = torch.empty(lib.sage_splitkv_workspace_bytes(B, Hq, M, D, num_splits), dtype=torch.uint8, device=q.device)
            L.check(lib.sage_attn_fusedq_pv_f4_splitkv_paged(
                L.desc(q, tensor_layout), L.dtype_code(q.dtype), L.desc(k8, tensor_layout), _img_desc(v4), L.desc(o, tensor_layout),
                L.dtype_code(o.dtype), k_scale.data_ptr(), km.data_ptr(), v4_scale.data_ptr(), L.ptr(lse), B, Hq, Hk, M, D,
                core._GRAN_CODE[qk_quant_gran], 32, float(sm_scale), *_table_args(block_table, page_size, P), kv_lens.data_ptr(),
                num_splits, int(causal), int(q_fold), ws.data_ptr(), ws.numel(), L.stream_ptr(q.device)),
                "sage_attn_fusedq_pv_f4_splitkv_paged")
        return (o, lse) if with_lse else o

    def fake(q, k8, k_scale, km, v4, v4_scale, block_table, kv_lens, num_splits, *rest):
        o = q.new_empty(q.shape)
        if not with_lse:
            return o
        B, Hq, M, _ = L.dims(q, rest[-3])
        return o, q.new_empty((B, Hq, M), dtype=torch.float32)

    op = torch.library.custom_op(f"{_NS}::{name}", body, mutates_args=(),
                                 schema=f"({params}) -> {'(Tensor, Tensor)' if with_lse else 'Tensor'}")
    op.register_fake(fake)
    return op


attn_splitkv_paged_v4 = _register_attn("attn_splitkv_paged_v4", False, False)
attn_splitkv_paged_v4_lse = _register_attn("attn_splitkv_paged_v4_lse", False, True)
attn_splitkv_causal_paged_v4 = _register_attn("attn_splitkv_causal_paged_v4", True, False)
attn_splitkv_causal_paged_v4_lse = _register_attn("attn_splitkv_causal_paged_v4_lse", True, True)


# ---- the cache ----------------------------------------------------------------------------------------------------------------
class SagePagedKVCacheV4:
    """``SagePagedKVCache`` with V as an MXFP4 image per page.  ``prepare`` binds the caller's pools (``[P, Hk, page_size, D]``;
    NHD: ``[P, page_size, Hk, D]``), freezes ``km`` per sequence and writes every valid page; ``append`` brings K and the image
    up to date after rows were written into pages, in one launch.  After any sequence of appends every valid tile of the state
    equals the same tile of a ``SageKVCacheV4`` on the gathered tensors, bit for bit; no byte of an untouched tile or of a page
    the sequence does not name is written.

    State: the pools ``k8``, ``k_scale`` and per sequence ``km`` of ``SagePagedKVCache``; the pools ``v4`` (uint8
    ``[P, Hk, D, 32 * page_size / 64]``) and ``v4_scale`` (uint8 ``[P, Hk, page_size / 64, 2 * D]``), in these shapes for both
    layouts.  Nothing of V is frozen."""

    def __init__(self, kc: SagePagedKVCache, v4, v4_scale):
        self._kc, self.v4, self.v4_scale = kc, v4, v4_scale

    # the K half is a SagePagedKVCache without V state: its pools, its strings and its tensors are this cache's
    k = property(lambda self: self._kc.k)
    v = property(lambda self: self._kc.v)
    k8 = property(lambda self: self._kc.k8)
    k_scale = property(lambda self: self._kc.k_scale)
    km = property(lambda self: self._kc.km)
    qk_quant_gran = property(lambda self: self._kc.qk_quant_gran)
    tensor_layout = property(lambda self: self._kc.tensor_layout)
    page_size = property(lambda self: self._kc.page_size)

    @classmethod
    def prepare(cls, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, kv_lens: torch.Tensor,
                qk_quant_gran: str = "per_thread", tensor_layout: str = "HND") -> "SagePagedKVCacheV4":
        """Bind the pools and prepare the first ``len_b`` rows of every sequence of ``block_table``.  The K half is
        ``SagePagedKVCache.prepare`` itself -- its checks (head_dim 64 or 128, page size 64, 128 or 256, aligned pools of one
        dtype and shape), one gather of the valid prefixes and the length-aware K pre-pass for ``km``; the pools of the image
        start as zero nibbles and scale bytes 127, so that a tile no call has written decodes to zeros, and one paged append
        from 0 writes every valid page."""
        kc = SagePagedKVCache.prepare(k_pool, v_pool, block_table, kv_lens, "fp16", qk_quant_gran, tensor_layout)
        P, Hk, page_size, D = L.dims(k_pool, tensor_layout)
        tpp = page_size // 64
        cache = cls(kc, torch.zeros((P, Hk, D, 32 * tpp), dtype=torch.uint8, device=k_pool.device),
                    torch.full((P, Hk, tpp, 2 * D), 127, dtype=torch.uint8, device=k_pool.device))
        cache._write_all(block_table, kv_lens)
        return cache

    def _write_all(self, block_table, kv_lens):
        kv_lens = core._check_kv_lens(kv_lens, self.km.size(0), self.k.device)
        self.append(block_table, torch.zeros_like(kv_lens), kv_lens, block_table.size(1) * self.page_size)

    def prepare_(self, block_table: torch.Tensor, kv_lens: torch.Tensor) -> "SagePagedKVCacheV4":
        """Prepare again from the bound pools at these lengths: a new frozen ``km`` (``SagePagedKVCache.prepare_``), then every
        valid page written by one paged append from 0.  On a ``narrow``-ed cache ``block_table`` holds the rows of its
        sequences alone, and only their pages and statistics are written."""
        self._kc.prepare_(block_table, kv_lens)
        self._write_all(block_table, kv_lens)
        return self

    def append(self, block_table: torch.Tensor, start_lens: torch.Tensor, kv_lens: torch.Tensor, max_new: int) -> None:
        """``SageKVCacheV4.append`` in logical tiles: ONE launch that re-quantizes K and the image of the 64-key tiles from the
        one holding row ``min(start_b, len_b - 1)`` to the last of ``len_b`` rows, each in the page ``block_table`` names.
        ``start_b >= len_b`` (no new rows, or a rollback) re-quantizes exactly the ragged tile; a sequence without keys touches
        nothing.  ``max_new`` (host int >= 1) bounds ``len_b - start_b`` over the sequences and sizes the grid."""
        if isinstance(max_new, bool) or not isinstance(max_new, int):
            raise TypeError(f"max_new must be an int >= 1, got {type(max_new).__name__}")
        if max_new < 1:
            raise ValueError(f"max_new must be >= 1, got {max_new}")
        B = self.km.size(0)
        block_table = _check_block_table(block_table, B, self.k.device)
        start_lens = core._check_kv_lens(start_lens, B, self.k.device)
        kv_lens = core._check_kv_lens(kv_lens, B, self.k.device)
        torch.ops.sageattention_amd_paged_fp4.kv_cache_append_paged_v4(
            self.k, self.v, self.km, self.k8, self.k_scale, self.v4, self.v4_scale, block_table, start_lens, kv_lens, max_new,
            self.tensor_layout, self.qk_quant_gran)

    def narrow(self, b0: int, nb: int) -> "SagePagedKVCacheV4":
        """A cache over the sequences ``[b0, b0 + nb)`` that shares the pools and ``km``'s storage with this one"""
        return SagePagedKVCacheV4(self._kc.narrow(b0, nb), self.v4, self.v4_scale)


def sageattn_splitkv_paged_v4(q: torch.Tensor, cache: SagePagedKVCacheV4, block_table: torch.Tensor, kv_lens: torch.Tensor,
                              num_splits: Optional[int] = None, causal: bool = False, q_fold: int = 1,
                              sm_scale: Optional[float] = None, return_lse: bool = False, **refused: Any):
    """``sageattn_splitkv_v4`` on a ``SagePagedKVCacheV4``: the paged attention launch over the splits -- P.V on the MXFP4 image
    out of the pages -- and the merge, no pre-pass and no gather.  o and lse are bit-identical to ``sageattn_splitkv_v4`` on a
    ``SageKVCacheV4`` over the padded tensors gathered from the pages, for every ``num_splits``, ``causal`` with ``q_fold``
    included; lse equals the paged FP8 cache's on the same K.  Table entries at or beyond ``ceil(len_b / page_size)`` influence
    nothing; a sequence without keys gives o = 0, lse = -inf.  The argument checks and the refusals by name are those of
    ``sageattn_splitkv_paged``."""
    if not isinstance(cache, SagePagedKVCacheV4):
        raise TypeError(f"cache must be a SagePagedKVCacheV4, got {type(cache).__name__}")
    if isinstance(causal, torch.Tensor) or not isinstance(causal, (bool, int)):
        raise TypeError(f"causal must be a bool, got {type(causal).__name__}")
    causal = bool(causal)
    op_name = "sageattn_splitkv_causal" if causal else "sageattn_splitkv"
    kc = cache._kc
    block_table = _check_block_table(block_table, q.size(0), kc.device)
    if kv_lens is None:
        raise TypeError("kv_lens must be an int32 tensor of shape [B]")
    kv_lens, ns, M = core._splitkv_front(op_name, causal, q, kc.k, kc.v, kv_lens, num_splits, kc.tensor_layout, "fp8",
                                         kc.qk_quant_gran, refused)
    if isinstance(q_fold, bool) or not isinstance(q_fold, int):
        raise TypeError(f"q_fold must be an int >= 1, got {type(q_fold).__name__}")
    if q_fold < 1 or M % q_fold != 0 or (q_fold != 1 and not causal):
        raise ValueError(f"q_fold must be >= 1 and divide the {M} query rows (and 1 unless causal), got {q_fold}")
    if q.dtype != kc.dtype or q.device != kc.device:
        raise ValueError("q must have the dtype and device of the cache's k")
    D = kc.head_dim
    if q.size(-1) != D:
        raise ValueError(f"q must have the cache's head_dim {D}, got {q.size(-1)}")
    B, Hq = L.dims(q, kc.tensor_layout)[:2]
    Hk = kc.num_kv_heads
    if Hq % Hk != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({Hk})")
    if kc.km.size(0) != B:
        raise ValueError(f"q has {B} sequences, the cache {kc.km.size(0)}")
    if num_splits is None:  # (from the logical capacity: the pool's third dim is one page)
        ns = core.splitkv_num_splits(B, Hq, M, block_table.size(1) * kc.page_size)
    if sm_scale is None:
        sm_scale = D ** -0.5
    fold = (q_fold,) if causal else ()
    op = getattr(torch.ops.sageattention_amd_paged_fp4,
                 f"attn_splitkv{'_causal' if causal else ''}_paged_v4{'_lse' if return_lse else ''}")
    return op(q, kc.k8, kc.k_scale, kc.km, cache.v4, cache.v4_scale, block_table, kv_lens, ns, *fold, kc.tensor_layout,
              float(sm_scale), kc.qk_quant_gran)
