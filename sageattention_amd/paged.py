"""A paged quantized KV cache for the split-KV operators: ``SageKVCache`` (kvcache.py) stored in fixed-size pages of one pool
and addressed through a per-sequence block table, as vLLM, SGLang and FlashAttention's ``block_table=`` keep their caches
(include/sageattn_hip_paged.h holds the rule).

The K scale groups and the blocks of the V^T image are 64-key tiles and both frozen statistics -- the smoothing vector ``km``
and the FP8 V scale -- are per sequence, so for a page size that is a multiple of 64 keys a page's quantized bytes depend on
the page's own rows and the sequence's statistics only: paging is an addressing change.  Every tile of the paged state and
every o / lse of ``sageattn_splitkv_paged`` is bit-identical to ``SageKVCache`` / ``sageattn_splitkv_cached`` on the padded
tensors gathered from the pages.

The block table is passed on every call and is not stored; it and the lengths are read on the device only, so
{append; attention} captures into one HIP graph and a replay reads what the tensors hold then.  The ops live in a namespace
of their own, ``torch.ops.sageattention_amd_paged``: ``kv_cache_append_paged`` (it mutates the state pools) and
``attn_splitkv_paged[_lse]`` / ``attn_splitkv_causal_paged[_lse]``; everything traces under ``torch.compile(fullgraph=True)``.

A cache that owns every pool and keeps no fp16 K pool is ``SagePagedRowCache`` (paged_rows.py).

Not built: page sizes below 64 (a 16-key page cannot hold a scale group), paged forms of the dense, ``kvlen`` and block-sparse
operators, and moving frozen statistics without preparing again.  Pages are not shared between sequences -- the frozen
statistics are per sequence; a prefix the sequences share is a sequence of its own: ``sageattn_splitkv_paged_prefix``
(prefix.py, include/sageattn_hip_prefix.h)."""
from typing import Any, Optional

import torch

from . import _lib as L
from . import core

__all__ = ["SagePagedKVCache", "sageattn_splitkv_paged"]

_NS = "sageattention_amd_paged"
PAGE_SIZES = (64, 128, 256)


def _check_page_size(page_size):
    if page_size not in PAGE_SIZES:
        raise ValueError(f"page_size must be 64, 128 or 256, got {page_size}: the K scale groups and the blocks of the V^T image "
                         "are 64-key tiles, so a page is a whole number of them")


def _check_block_table(block_table, B, device):
    """``block_table`` as the kernels read it: int32 [B, max_pages >= 1] (B None: any) on the device with a contiguous last
    dim (its values stay on the device; a row stride beyond max_pages is passed on)"""
    if not isinstance(block_table, torch.Tensor):
        raise TypeError("block_table must be an int32 tensor of shape [B, max_pages]")
    if block_table.dtype != torch.int32:
        raise TypeError(f"block_table must be of dtype int32, got {block_table.dtype}")
    if block_table.dim() != 2 or block_table.size(0) < 1 or block_table.size(1) < 1 or B not in (None, block_table.size(0)):
        raise ValueError(f"block_table shape {tuple(block_table.shape)} does not match "
                         f"[B{'' if B is None else '=' + str(B)}, max_pages >= 1]")
    B = block_table.size(0)
    if block_table.device != device:
        raise ValueError(f"block_table is on {block_table.device}, the pools on {device}")
    if block_table.stride(1) != 1 or (B > 1 and block_table.stride(0) < block_table.size(1)):
        raise ValueError("block_table must have a contiguous last dim (stride(-1) == 1) and rows that do not overlap")
    return block_table


def _table_args(block_table, page_size, num_pages):
    """block_table table_stride max_pages page_size num_pages of the C signatures"""
    stride = block_table.stride(0) if block_table.size(0) > 1 else max(block_table.stride(0), block_table.size(1))
    return block_table.data_ptr(), stride, block_table.size(1), page_size, num_pages


# ---- ops ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::kv_cache_append_paged", mutates_args=("k8", "k_scale", "v8"))
def kv_cache_append_paged(k: torch.Tensor, v: Optional[torch.Tensor], km: torch.Tensor, k8: torch.Tensor, k_scale: torch.Tensor,
                          v8: Optional[torch.Tensor], v_coef: Optional[torch.Tensor], block_table: torch.Tensor,
                          start_lens: torch.Tensor, kv_lens: torch.Tensor, max_new: int, tensor_layout: str,
                          qk_quant_gran: str) -> None:
    """sage_kv_cache_append_paged on the pools of a cache: one launch; ``v8`` None: no V half"""
    P, H, page_size, D = L.dims(k, tensor_layout)
    gran, rnd = core._k_pairing(qk_quant_gran)
    with torch.cuda.device(k.device):
        L.check(L.lib().sage_kv_cache_append_paged(
            L.desc(k, tensor_layout), None if v8 is None else L.desc(v, tensor_layout), L.dtype_code(k.dtype),
            block_table.size(0), H, D, km.data_ptr(), L.desc(k8, tensor_layout), k_scale.data_ptr(), gran, rnd,
            None if v8 is None else L.desc_vt(v8, tensor_layout), L.ptr(v_coef), *_table_args(block_table, page_size, P),
            start_lens.data_ptr(), kv_lens.data_ptr(), int(max_new), L.stream_ptr(k.device)), "sage_kv_cache_append_paged")


@kv_cache_append_paged.register_fake
def _(k, v, km, k8, k_scale, v8, v_coef, block_table, start_lens, kv_lens, max_new, tensor_layout, qk_quant_gran):
    return None


def _register_attn(name, causal, with_lse):
    """attn_splitkv[_causal]_paged[_lse]: sage_attn_fusedq_pv_{f16,f8}_splitkv_paged on the pools of a cache (``v``: the fp16 /
    bf16 V pool, or with a ``v_scale`` the pool of V^T images); num_splits 0 = ``core.splitkv_num_splits`` on the logical
    capacity; o is contiguous in q's shape"""
    params = ("Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor block_table, Tensor kv_lens, "
              "SymInt num_splits, " + "SymInt q_fold, " * causal + "str tensor_layout, float sm_scale, str qk_quant_gran")

    def body(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, num_splits, *rest):
        q_fold = rest[0] if causal else 1
        tensor_layout, sm_scale, qk_quant_gran = rest[-3:]
        B, Hq, M, D = L.dims(q, tensor_layout)
        P, Hk, page_size, _ = L.dims(k8, tensor_layout)
        num_splits = num_splits or core.splitkv_num_splits(B, Hq, M, block_table.size(1) * page_size)
        lib = L.lib()
        pv_fp8 = v_scale is not None
        with torch.cuda.device(q.device):
            q = core._abi_view(q)  # (a view the C ABI cannot address travels as a contiguous copy, as in the operators)
            o = torch.empty(q.size(), dtype=q.dtype, device=q.device)
            lse = torch.empty((B, Hq, M), dtype=torch.float32, device=q.device) if with_lse else None
            ws = torch.empty(lib.sage_splitkv_workspace_bytes(B, Hq, M, D, num_splits), dtype=torch.uint8, device=q.device)
            fn = f"sage_attn_fusedq_pv_{'f8' if pv_fp8 else 'f16'}_splitkv_paged"
            # in the order of the C signatures: the f8 form has no v_dtype and takes v_scale
            v_args = (L.desc_vt(v, tensor_layout),) if pv_fp8 else (L.desc(v, tensor_layout), L.dtype_code(v.dtype))
            L.check(getattr(lib, fn)(
                L.desc(q, tensor_layout), L.dtype_code(q.dtype), L.desc(k8, tensor_layout), *v_args, L.desc(o, tensor_layout),
                L.dtype_code(o.dtype), k_scale.data_ptr(), km.data_ptr(), *((v_scale.data_ptr(),) if pv_fp8 else ()), L.ptr(lse),
                B, Hq, Hk, M, D, core._GRAN_CODE[qk_quant_gran], 32, float(sm_scale), *_table_args(block_table, page_size, P),
                kv_lens.data_ptr(), num_splits, int(causal), int(q_fold), ws.data_ptr(), ws.numel(), L.stream_ptr(q.device)), fn)
        return (o, lse) if with_lse else o

    def fake(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, num_splits, *rest):
        tensor_layout = rest[-3]
        o = q.new_empty(q.shape)
        if not with_lse:
            return o
        B, Hq, M, _ = L.dims(q, tensor_layout)
        return o, q.new_empty((B, Hq, M), dtype=torch.float32)

    op = torch.library.custom_op(f"{_NS}::{name}", body, mutates_args=(),
                                 schema=f"({params}) -> {'(Tensor, Tensor)' if with_lse else 'Tensor'}")
    op.register_fake(fake)
    return op


attn_splitkv_paged = _register_attn("attn_splitkv_paged", False, False)
attn_splitkv_paged_lse = _register_attn("attn_splitkv_paged_lse", False, True)
attn_splitkv_causal_paged = _register_attn("attn_splitkv_causal_paged", True, False)
attn_splitkv_causal_paged_lse = _register_attn("attn_splitkv_causal_paged_lse", True, True)


# ---- the cache ----------------------------------------------------------------------------------------------------------------
class SagePagedKVCache:
    """Prepared split-KV operands of a KV cache kept in pages: ``k_pool`` / ``v_pool`` are ``[P, Hk, page_size, D]`` (HND; NHD:
    ``[P, page_size, Hk, D]``), and row b of a ``block_table`` (int32 ``[B, max_pages]``, passed on every call) names the pages
    of sequence b: entries ``[0, ceil(len_b / page_size))`` are page ids in ``[0, P)``, ``len_b = clamp(kv_lens[b], 0,
    max_pages * page_size)``.  Entries beyond are never used, and the valid pages of different sequences must be distinct.

    ``prepare`` binds the pools -- the caller goes on writing rows into pages -- freezes the statistics of every sequence and
    quantizes its valid pages; ``append`` brings the state up to date after rows were written.  The rule is that of
    ``SageKVCache`` in logical 64-key tiles (include/sageattn_hip_paged.h): after any sequence of appends every valid tile of
    the state equals the same tile of a ``SageKVCache`` on the gathered tensors, bit for bit.

    State: the pools ``k8`` (INT8, shaped as ``k_pool``) and ``k_scale`` (fp32 ``[P, Hk, (page_size/64) * g]``, g = 4 per-thread,
    1 per-block); per sequence ``km`` ``[B, Hk, D]``; FP8 P.V: the pool ``v8`` of V^T images per page (``[P, Hk, D, page_size]``;
    NHD: ``[P, D, Hk, page_size]``) and per sequence ``v_scale``, ``v_coef``.  FP16 / BF16 P.V keeps no V state."""

    def __init__(self, k_pool, v_pool, pv, qk_quant_gran, tensor_layout, v_headroom):
        self.k, self.v, self.pv, self.qk_quant_gran, self.tensor_layout = k_pool, v_pool, pv, qk_quant_gran, tensor_layout
        self.v_headroom = v_headroom
        self.page_size = L.dims(k_pool, tensor_layout)[2]
        self.k8 = self.k_scale = self.km = self.v8 = self.v_scale = self.v_coef = None

    # what sageattn_splitkv_paged reads of a cache
    dtype = property(lambda self: self.k.dtype)
    device = property(lambda self: self.k.device)
    head_dim = property(lambda self: self.k.size(-1))
    num_kv_heads = property(lambda self: L.dims(self.k, self.tensor_layout)[1])

    @classmethod
    def prepare(cls, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, kv_lens: torch.Tensor,
                pv: str = "fp16", qk_quant_gran: str = "per_thread", tensor_layout: str = "HND",
                v_headroom: float = 2.0) -> "SagePagedKVCache":
        """Bind the pools and prepare the first ``len_b`` rows of every sequence of ``block_table``.  The statistics come from
        the existing length-aware pre-pass on a padded copy gathered ONCE from the valid pages (paid per sequence or serving
        slot, not per step); the pages are then written by one paged append from 0.  head_dim must be 64 or 128, the page
        size 64, 128 or 256, and the pools 16-byte aligned with strides that are multiples of 16 bytes: the cache binds them
        and cannot take a copy."""
        core._check_sparse_args(pv, qk_quant_gran, tensor_layout)
        if isinstance(v_headroom, bool) or not isinstance(v_headroom, (int, float)):
            raise TypeError(f"v_headroom must be a float >= 1, got {type(v_headroom).__name__}")
        if not v_headroom >= 1:
            raise ValueError(f"v_headroom must be >= 1, got {v_headroom}")
        if k_pool.dim() != 4 or v_pool.dim() != 4:
            raise ValueError("k_pool and v_pool must be 4-D")
        if k_pool.size(-1) not in (64, 128) or v_pool.size(-1) != k_pool.size(-1):
            raise ValueError(f"SagePagedKVCache needs head_dim 64 or 128 (no padded copy: the cache binds the pools), got "
                             f"{k_pool.size(-1)} and {v_pool.size(-1)}")
        if k_pool.dtype not in (torch.float16, torch.bfloat16) or v_pool.dtype != k_pool.dtype or v_pool.device != k_pool.device:
            raise ValueError("k_pool and v_pool must be fp16 or bf16 tensors of one dtype on one device")
        if k_pool.shape != v_pool.shape:
            raise ValueError(f"k_pool and v_pool must have one shape, got {tuple(k_pool.shape)} and {tuple(v_pool.shape)}")
        _check_page_size(L.dims(k_pool, tensor_layout)[2])
        if (k_pool.stride(-1) != 1 or v_pool.stride(-1) != 1 or core._abi_view(k_pool) is not k_pool
                or core._abi_view(v_pool) is not v_pool):
            raise ValueError("k_pool and v_pool must be 16-byte aligned with a contiguous last dim and strides that are "
                             "multiples of 16 bytes: the cache binds the pools and cannot take a copy")
        cache = cls(k_pool, v_pool, pv, qk_quant_gran, tensor_layout, float(v_headroom))
        block_table = _check_block_table(block_table, None, k_pool.device)
        kv_lens = core._check_kv_lens(kv_lens, block_table.size(0), k_pool.device)
        P, Hk, page_size, D = L.dims(k_pool, tensor_layout)
        B = block_table.size(0)
        dev = k_pool.device
        g = 4 if qk_quant_gran == "per_thread" else 1
        cache.k8 = torch.empty(k_pool.shape, dtype=torch.int8, device=dev)
        cache.k_scale = torch.empty((P, Hk, page_size // 64 * g), dtype=torch.float32, device=dev)
        cache.km = torch.empty((B, Hk, D), dtype=k_pool.dtype, device=dev)
        if pv == "fp8":
            shape = (P, Hk, D, page_size) if tensor_layout == "HND" else (P, D, Hk, page_size)
            cache.v8 = torch.empty(shape, dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
            cache.v_scale = torch.empty((B, Hk, D), dtype=torch.float32, device=dev)
            cache.v_coef = torch.empty((B, Hk, 2, D), dtype=torch.float32, device=dev)
        cache.prepare_(block_table, kv_lens)
        return cache

    def _gather(self, pool, block_table, kv_lens):
        """the padded [B,Hk,N,D] (NHD: [B,N,Hk,D]) copy of the sequences' pages in table order.  Entries at or beyond
        ceil(len_b / page_size) are not used as indices (page 0 stands in; the length-aware pre-pass loads none of its rows)."""
        B, max_pages = block_table.shape
        need = (kv_lens.clamp(0, max_pages * self.page_size) + (self.page_size - 1)) // self.page_size
        valid = torch.arange(max_pages, device=block_table.device).unsqueeze(0) < need.unsqueeze(1)
        x = pool[torch.where(valid, block_table, torch.zeros_like(block_table)).long()]   # [B, max_pages, (page)]
        if self.tensor_layout == "HND":
            x = x.permute(0, 2, 1, 3, 4)                                                   # [B, Hk, max_pages, page_size, D]
            return x.reshape(B, x.size(1), max_pages * self.page_size, x.size(4))
        return x.reshape(B, max_pages * self.page_size, x.size(3), x.size(4))

    def prepare_(self, block_table: torch.Tensor, kv_lens: torch.Tensor) -> "SagePagedKVCache":
        """Prepare again from the bound pools at these lengths: new frozen statistics, then every valid page written by one
        paged append from 0.  On a ``narrow``-ed cache ``block_table`` holds the rows of its sequences alone, and only their
        pages and statistics are written."""
        B = self.km.size(0)
        block_table = _check_block_table(block_table, B, self.k.device)
        kv_lens = core._check_kv_lens(kv_lens, B, self.k.device)
        fp8 = self.pv == "fp8"
        with torch.cuda.device(self.k.device):
            kg = self._gather(self.k, block_table, kv_lens)
            vg = self._gather(self.v, block_table, kv_lens) if fp8 else kg
            _, _, km, _, v_scale, _ = core._prepass(kg, vg, self.tensor_layout, self.qk_quant_gran, True, fp8, False, kv_lens)
            self.km.copy_(km)
            if fp8:
                v_scale_c = v_scale * self.v_headroom            # fp32 product
                self.v_scale.copy_(v_scale_c)
                self.v_coef[:, :, 0] = 0
                self.v_coef[:, :, 1] = torch.where(v_scale_c == 0, torch.zeros_like(v_scale_c), 1.0 / v_scale_c)
            self.append(block_table, torch.zeros_like(kv_lens), kv_lens, block_table.size(1) * self.page_size)
        return self

    def append(self, block_table: torch.Tensor, start_lens: torch.Tensor, kv_lens: torch.Tensor, max_new: int) -> None:
        """Bring the state up to date after the caller wrote rows ``[start_lens[b], kv_lens[b])`` of the sequences into their
        pages: ONE launch, the rule of ``SageKVCache.append`` in logical tiles -- a slot looks its page up in ``block_table``.
        ``start_b >= len_b`` adds no rows (or follows a rollback) and re-quantizes exactly the tile holding row ``len_b - 1``.
        ``max_new`` (host int >= 1) bounds ``len_b - start_b`` over the sequences and sizes the grid.  No byte of a tile that is
        not touched and no byte of a page the sequence does not name is written."""
        if isinstance(max_new, bool) or not isinstance(max_new, int):
            raise TypeError(f"max_new must be an int >= 1, got {type(max_new).__name__}")
        if max_new < 1:
            raise ValueError(f"max_new must be >= 1, got {max_new}")
        B = self.km.size(0)
        block_table = _check_block_table(block_table, B, self.k.device)
        start_lens = core._check_kv_lens(start_lens, B, self.k.device)
        kv_lens = core._check_kv_lens(kv_lens, B, self.k.device)
        fp8 = self.pv == "fp8"
        torch.ops.sageattention_amd_paged.kv_cache_append_paged(
            self.k, self.v if fp8 else None, self.km, self.k8, self.k_scale, self.v8, self.v_coef, block_table, start_lens,
            kv_lens, max_new, self.tensor_layout, self.qk_quant_gran)

    def narrow(self, b0: int, nb: int) -> "SagePagedKVCache":
        """A cache over the sequences ``[b0, b0 + nb)`` that shares the pools and the per-sequence statistics' storage with
        this one: ``prepare_(block_table_rows, kv_lens)`` on it re-prepares those serving slots alone."""
        c = SagePagedKVCache(self.k, self.v, self.pv, self.qk_quant_gran, self.tensor_layout, self.v_headroom)
        c.k8, c.k_scale, c.v8 = self.k8, self.k_scale, self.v8
        for name in ("km", "v_scale", "v_coef"):
            t = getattr(self, name)
            setattr(c, name, None if t is None else t.narrow(0, b0, nb))
        return c


_CACHE_TYPES = [SagePagedKVCache]  # ... and SagePagedRowCache (paged_rows.py), whose pools the same kernels read


def sageattn_splitkv_paged(q: torch.Tensor, cache: SagePagedKVCache, block_table: torch.Tensor, kv_lens: torch.Tensor,
                           num_splits: Optional[int] = None, causal: bool = False, q_fold: int = 1,
                           sm_scale: Optional[float] = None, return_lse: bool = False, **refused: Any):
    """``sageattn_splitkv_cached`` on a ``SagePagedKVCache``: the paged attention launch over the splits and the merge, no
    pre-pass and no gather.  o and lse are bit-identical to ``sageattn_splitkv_cached`` on a ``SageKVCache`` over the padded
    tensors gathered from the pages, with the same ``kv_lens``, ``num_splits``, ``causal`` and ``q_fold``: the split ranges
    follow ``len_b`` in 64-key tiles and do not depend on the page size.  Rows at or beyond ``len_b`` of the last page and
    table entries at or beyond ``ceil(len_b / page_size)`` influence nothing; a sequence without keys gives o = 0, lse = -inf.

    ``num_splits``: 1..16, or None for ``splitkv_num_splits(B, Hq, M, max_pages * page_size)``; 1 runs the paged split kernel
    with one split.  What ``sageattn_splitkv_cached`` refuses is refused here in the same words."""
    if not isinstance(cache, tuple(_CACHE_TYPES)):
        raise TypeError(f"cache must be a SagePagedKVCache, got {type(cache).__name__}")
    if isinstance(causal, torch.Tensor) or not isinstance(causal, (bool, int)):
        raise TypeError(f"causal must be a bool, got {type(causal).__name__}")
    causal = bool(causal)
    op_name = "sageattn_splitkv_causal" if causal else "sageattn_splitkv"
    block_table = _check_block_table(block_table, q.size(0), cache.device)
    # (shapes only: a cache without fp16 pools has its INT8 K pool in their shape)
    k_like, v_like = (cache.k, cache.v) if isinstance(cache, SagePagedKVCache) else (cache.k8, cache.k8)
    if kv_lens is None:
        raise TypeError("kv_lens must be an int32 tensor of shape [B]")
    kv_lens, ns, M = core._splitkv_front(op_name, causal, q, k_like, v_like, kv_lens, num_splits, cache.tensor_layout,
                                         cache.pv, cache.qk_quant_gran, refused)
    if isinstance(q_fold, bool) or not isinstance(q_fold, int):
        raise TypeError(f"q_fold must be an int >= 1, got {type(q_fold).__name__}")
    if q_fold < 1 or M % q_fold != 0 or (q_fold != 1 and not causal):
        raise ValueError(f"q_fold must be >= 1 and divide the {M} query rows (and 1 unless causal), got {q_fold}")
    if q.dtype != cache.dtype or q.device != cache.device:
        raise ValueError("q must have the dtype and device of the cache's k")
    D = cache.head_dim
    if q.size(-1) != D:
        raise ValueError(f"q must have the cache's head_dim {D}, got {q.size(-1)}")
    B, Hq = L.dims(q, cache.tensor_layout)[:2]
    Hk = cache.num_kv_heads
    if Hq % Hk != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({Hk})")
    if cache.km.size(0) != B:
        raise ValueError(f"q has {B} sequences, the cache {cache.km.size(0)}")
    if num_splits is None:  # (from the logical capacity: the pool's third dim is one page)
        ns = core.splitkv_num_splits(B, Hq, M, block_table.size(1) * cache.page_size)
    if sm_scale is None:
        sm_scale = D ** -0.5
    fp8 = cache.pv == "fp8"
    fold = (q_fold,) if causal else ()
    op = getattr(torch.ops.sageattention_amd_paged,
                 f"attn_splitkv{'_causal' if causal else ''}_paged{'_lse' if return_lse else ''}")
    return op(q, cache.k8, cache.k_scale, cache.km, cache.v8 if fp8 else cache.v, cache.v_scale if fp8 else None, block_table,
              kv_lens, ns, *fold, cache.tensor_layout, float(sm_scale), cache.qk_quant_gran)
