"""The paged quantized KV cache without fp16 pools: ``SagePagedKVCache`` (paged.py) binds the caller's fp16 ``k_pool`` and
``v_pool`` and keeps its quantized pools beside them; ``SagePagedRowCache`` owns every pool and takes the step's new K / V rows
``[B, Hk, T, D]`` as arguments, as a serving engine holds them after the projection (include/sageattn_hip_paged_rows.h holds the
rule).

The attention kernels never read fp16 K, and with FP8 P.V no fp16 V.  Only the append does: a K scale group is a maximum over
the rows of a 64-key tile, and a new row can move it.  So the cache keeps the fp16 rows of the CURRENT tile per sequence and
head -- ``k_tail``, a ring of two tile slots -- and nothing else of fp16 K.  V is quantized element by element under frozen
coefficients and needs no tail.  Per cached key and KV head at head_dim 128 that is 256.25 bytes with FP8 P.V (fp16 cache:
512, ``SagePagedKVCache`` with its bound pools: 768.25) and 384.25 with FP16 P.V (512, 640.25), plus the tail.

Every tile of the state and every o / lse of ``sageattn_splitkv_paged`` on it is bit-identical to ``SagePagedKVCache`` over
fp16 pools into which the same rows were written.  The table and the lengths are read on the device only: {append_rows;
attention} captures into one HIP graph.  The op lives in a namespace of its own,
``torch.ops.sageattention_amd_paged_rows.kv_cache_append_rows_paged`` (it mutates the pools and the tail), and traces under
``torch.compile(fullgraph=True)``.

Not built: the same for the contiguous ``SageKVCache`` and moving frozen statistics without preparing again.  A prefix the
sequences share is a sequence of its own: ``sageattn_splitkv_paged_prefix`` (prefix.py)."""
from typing import Optional

import torch

from . import _lib as L
from . import core
from . import paged

__all__ = ["SagePagedRowCache"]

_NS = "sageattention_amd_paged_rows"


@torch.library.custom_op(f"{_NS}::kv_cache_append_rows_paged", mutates_args=("k_tail", "k8", "k_scale", "v_pool", "v8"))
def kv_cache_append_rows_paged(k_new: torch.Tensor, v_new: torch.Tensor, km: torch.Tensor, k_tail: torch.Tensor,
                               k8: torch.Tensor, k_scale: torch.Tensor, v_pool: Optional[torch.Tensor],
                               v8: Optional[torch.Tensor], v_coef: Optional[torch.Tensor], block_table: torch.Tensor,
                               start_lens: torch.Tensor, kv_lens: torch.Tensor, tensor_layout: str, qk_quant_gran: str) -> None:
    """sage_kv_cache_append_rows_paged on the pools of a cache: one launch; exactly one of ``v_pool`` / ``v8`` is given"""
    B, H, T, D = L.dims(k_new, tensor_layout)
    P, _, page_size, _ = L.dims(k8, tensor_layout)
    gran, rnd = core._k_pairing(qk_quant_gran)
    with torch.cuda.device(k8.device):
        # (a view the C ABI cannot address travels as a contiguous copy, as in the operators)
        k_new, v_new = core._abi_view(k_new), core._abi_view(v_new)
        L.check(L.lib().sage_kv_cache_append_rows_paged(
            L.desc(k_new, tensor_layout), L.desc(v_new, tensor_layout), L.dtype_code(k_new.dtype), B, H, T, D, km.data_ptr(),
            k_tail.data_ptr(), L.desc(k8, tensor_layout), k_scale.data_ptr(), gran, rnd,
            None if v_pool is None else L.desc(v_pool, tensor_layout), None if v8 is None else L.desc_vt(v8, tensor_layout),
            L.ptr(v_coef), *paged._table_args(block_table, page_size, P), start_lens.data_ptr(), kv_lens.data_ptr(),
            L.stream_ptr(k8.device)), "sage_kv_cache_append_rows_paged")


@kv_cache_append_rows_paged.register_fake
def _(k_new, v_new, km, k_tail, k8, k_scale, v_pool, v8, v_coef, block_table, start_lens, kv_lens, tensor_layout, qk_quant_gran):
    return None


class SagePagedRowCache:
    """Prepared split-KV operands of a paged KV cache that owns all its storage.  Row b of a ``block_table`` (int32
    ``[B, max_pages]``, passed on every call) names the pages of sequence b, as for ``SagePagedKVCache``.

    State: the pools ``k8`` (INT8 ``[P, Hk, page_size, D]``; NHD: ``[P, page_size, Hk, D]``) and ``k_scale``; FP8 P.V: the pool
    ``v8`` of V^T images and per sequence ``v_scale``, ``v_coef``; FP16 / BF16 P.V: ``v_pool`` in the input dtype, shaped as
    ``k8``, which the cache fills; per sequence ``km`` and ``k_tail`` ``[B, Hk, 2, 64, D]`` in the input dtype: row r of a
    sequence lives in slot ``(r >> 6) & 1``, row ``r & 63``.  ``v`` is the V operand of the attention kernels (``v8`` or
    ``v_pool``)."""

    def __init__(self, pv, qk_quant_gran, tensor_layout, v_headroom, page_size, dtype):
        self.pv, self.qk_quant_gran, self.tensor_layout, self.v_headroom = pv, qk_quant_gran, tensor_layout, v_headroom
        self.page_size, self.dtype = page_size, dtype
        self.k8 = self.k_scale = self.km = self.k_tail = self.v_pool = self.v8 = self.v_scale = self.v_coef = None

    # what sageattn_splitkv_paged reads of a cache
    @property
    def device(self):
        return self.k8.device

    @property
    def head_dim(self):
        return self.k8.size(-1)

    @property
    def num_kv_heads(self):
        return L.dims(self.k8, self.tensor_layout)[1]

    @property
    def v(self):
        return self.v8 if self.pv == "fp8" else self.v_pool

    @classmethod
    def allocate(cls, num_pages: int, page_size: int, B: int, Hk: int, D: int, dtype: torch.dtype, device, pv: str = "fp16",
                 qk_quant_gran: str = "per_thread", tensor_layout: str = "HND", v_headroom: float = 2.0) -> "SagePagedRowCache":
        """The state of a cache of ``num_pages`` pages for ``B`` sequences, unprepared: ``prepare_`` fills it."""
        core._check_sparse_args(pv, qk_quant_gran, tensor_layout)
        if isinstance(v_headroom, bool) or not isinstance(v_headroom, (int, float)):
            raise TypeError(f"v_headroom must be a float >= 1, got {type(v_headroom).__name__}")
        if not v_headroom >= 1:
            raise ValueError(f"v_headroom must be >= 1, got {v_headroom}")
        for name, value in (("num_pages", num_pages), ("page_size", page_size), ("B", B), ("Hk", Hk), ("D", D)):
            if isinstance(value, bool) or not isinstance(value, int):
                raise TypeError(f"{name} must be an int, got {type(value).__name__}")
        paged._check_page_size(page_size)
        if D not in (64, 128):
            raise ValueError(f"SagePagedRowCache needs head_dim 64 or 128, got {D}")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        if num_pages < 1 or B < 1 or Hk < 1:
            raise ValueError(f"num_pages, B and Hk must be >= 1, got {num_pages}, {B}, {Hk}")
        c = cls(pv, qk_quant_gran, tensor_layout, float(v_headroom), page_size, dtype)
        hnd = tensor_layout == "HND"
        g = 4 if qk_quant_gran == "per_thread" else 1
        shape = (num_pages, Hk, page_size, D) if hnd else (num_pages, page_size, Hk, D)
        c.k8 = torch.empty(shape, dtype=torch.int8, device=device)
        c.k_scale = torch.empty((num_pages, Hk, page_size // 64 * g), dtype=torch.float32, device=device)
        c.km = torch.empty((B, Hk, D), dtype=dtype, device=device)
        c.k_tail = torch.empty((B, Hk, 2, 64, D), dtype=dtype, device=device)
        if pv == "fp8":
            vt = (num_pages, Hk, D, page_size) if hnd else (num_pages, D, Hk, page_size)
            c.v8 = torch.empty(vt, dtype=torch.uint8, device=device).view(torch.float8_e4m3fn)
            c.v_scale = torch.empty((B, Hk, D), dtype=torch.float32, device=device)
            c.v_coef = torch.empty((B, Hk, 2, D), dtype=torch.float32, device=device)
        else:
            c.v_pool = torch.empty(shape, dtype=dtype, device=device)
        return c

    @classmethod
    def prepare(cls, k: torch.Tensor, v: torch.Tensor, block_table: torch.Tensor, kv_lens: torch.Tensor, num_pages: int,
                page_size: int, pv: str = "fp16", qk_quant_gran: str = "per_thread", tensor_layout: str = "HND",
                v_headroom: float = 2.0) -> "SagePagedRowCache":
        """``allocate`` for the sequences of the padded prompt ``k`` / ``v``, then ``prepare_``"""
        if not isinstance(k, torch.Tensor) or k.dim() != 4:
            raise ValueError("k and v must be 4-D tensors")
        core._check_sparse_args(pv, qk_quant_gran, tensor_layout)
        B, Hk, _, D = L.dims(k, tensor_layout)
        c = cls.allocate(num_pages, page_size, B, Hk, D, k.dtype, k.device, pv=pv, qk_quant_gran=qk_quant_gran,
                         tensor_layout=tensor_layout, v_headroom=v_headroom)
        return c.prepare_(k, v, block_table, kv_lens)

    def _check_rows(self, k_new, v_new, what):
        """the rows of a call: ``[B, Hk, T, D]`` (NHD: ``[B, T, Hk, D]``) of the cache's dtype on its device -> B, T"""
        if not isinstance(k_new, torch.Tensor) or not isinstance(v_new, torch.Tensor):
            raise TypeError(f"{what} must be tensors")
        if k_new.dim() != 4 or v_new.dim() != 4:
            raise ValueError(f"{what} must be 4-D")
        if k_new.shape != v_new.shape:
            raise ValueError(f"{what} must have one shape, got {tuple(k_new.shape)} and {tuple(v_new.shape)}")
        if k_new.dtype != self.dtype or v_new.dtype != self.dtype:
            raise ValueError(f"{what} must have the cache's dtype {self.dtype}, got {k_new.dtype} and {v_new.dtype}")
        if k_new.device != self.device or v_new.device != self.device:
            raise ValueError(f"{what} are on {k_new.device} and {v_new.device}, the cache on {self.device}")
        B, Hk, T, D = L.dims(k_new, self.tensor_layout)
        if (B, Hk, D) != tuple(self.km.shape) or T < 1:
            raise ValueError(f"{what} shape {tuple(k_new.shape)} does not match B={self.km.size(0)}, Hk={self.km.size(1)}, "
                             f"T >= 1, head_dim {self.km.size(2)} of the cache in layout {self.tensor_layout}")
        if k_new.stride(-1) != 1 or v_new.stride(-1) != 1:
            raise ValueError(f"{what} must have a contiguous last dim (stride(-1) == 1)")
        return B, T

    def prepare_(self, k: torch.Tensor, v: torch.Tensor, block_table: torch.Tensor, kv_lens: torch.Tensor) -> "SagePagedRowCache":
        """Freeze the statistics of every sequence from the padded prompt ``k`` / ``v`` ``[B, Hk, N0, D]`` (``kv_lens[b] <= N0``
        rows of sequence b are valid; N0 at most the capacity ``max_pages * page_size``) by the length-aware pre-pass -- whose
        statistics are chunked by each sequence's own length and do not depend on N0 -- then write the pages and the tail by one
        ``append_rows`` from 0.  On a ``narrow``-ed cache the arguments are those of its sequences alone."""
        B, N0 = self._check_rows(k, v, "k and v")
        block_table = paged._check_block_table(block_table, B, self.device)
        kv_lens = core._check_kv_lens(kv_lens, B, self.device)
        if N0 > block_table.size(1) * self.page_size:
            raise ValueError(f"the prompt has {N0} rows, the table names {block_table.size(1)} pages of {self.page_size}: "
                             f"a capacity of {block_table.size(1) * self.page_size}")
        fp8 = self.pv == "fp8"
        with torch.cuda.device(self.device):
            k, v = core._abi_view(k), core._abi_view(v)
            _, _, km, _, v_scale, _ = core._prepass(k, v if fp8 else k, self.tensor_layout, self.qk_quant_gran, True, fp8, False,
                                                    kv_lens)
            self.km.copy_(km)
            if fp8:
                v_scale_c = v_scale * self.v_headroom            # fp32 product
                self.v_scale.copy_(v_scale_c)
                self.v_coef[:, :, 0] = 0
                self.v_coef[:, :, 1] = torch.where(v_scale_c == 0, torch.zeros_like(v_scale_c), 1.0 / v_scale_c)
            self._append(k, v, block_table, torch.zeros_like(kv_lens), kv_lens)
        return self

    def _append(self, k_new, v_new, block_table, start_lens, kv_lens):
        torch.ops.sageattention_amd_paged_rows.kv_cache_append_rows_paged(
            k_new, v_new, self.km, self.k_tail, self.k8, self.k_scale, self.v_pool, self.v8, self.v_coef, block_table, start_lens,
            kv_lens, self.tensor_layout, self.qk_quant_gran)

    def append_rows(self, k_new: torch.Tensor, v_new: torch.Tensor, block_table: torch.Tensor, start_lens: torch.Tensor,
                    kv_lens: torch.Tensor) -> None:
        """Append the rows ``k_new[b, :, :n_b]`` / ``v_new[b, :, :n_b]`` (``[B, Hk, T, D]``; NHD: ``[B, T, Hk, D]``; a strided view
        with a contiguous last dim is read in place when it is 16-byte aligned with strides that are multiples of 16 bytes) as
        the logical rows ``[start_lens[b], kv_lens[b])`` of the sequences, ``n_b = kv_lens[b] - start_lens[b] <= T``: ONE
        launch.  Rows at or beyond n_b are never loaded.  ``start_b >= len_b`` adds no rows -- or follows a rollback of up to 64
        rejected speculative rows -- and re-quantizes the tile holding row ``len_b - 1`` from the tail; ``start_b`` below the old
        length overwrites and extends.  The tail serves a call whose first touched tile is not more than one below the highest
        tile written since ``prepare_`` (not checked)."""
        B, _ = self._check_rows(k_new, v_new, "k_new and v_new")
        block_table = paged._check_block_table(block_table, B, self.device)
        start_lens = core._check_kv_lens(start_lens, B, self.device)
        kv_lens = core._check_kv_lens(kv_lens, B, self.device)
        self._append(k_new, v_new, block_table, start_lens, kv_lens)

    def narrow(self, b0: int, nb: int) -> "SagePagedRowCache":
        """A cache over the sequences ``[b0, b0 + nb)`` that shares the pools and the storage of the per-sequence state (the
        statistics and the tail) with this one: ``prepare_`` on it re-prepares those serving slots alone."""
        c = SagePagedRowCache(self.pv, self.qk_quant_gran, self.tensor_layout, self.v_headroom, self.page_size, self.dtype)
        c.k8, c.k_scale, c.v8, c.v_pool = self.k8, self.k_scale, self.v8, self.v_pool
        for name in ("km", "k_tail", "v_scale", "v_coef"):
            t = getattr(self, name)
            setattr(c, name, None if t is None else t.narrow(0, b0, nb))
        return c

    def nbytes(self) -> int:
        """bytes of all state: the pools, the statistics and the tail"""
        return sum(t.numel() * t.element_size() for t in (self.k8, self.k_scale, self.km, self.k_tail, self.v_pool, self.v8,
                                                          self.v_scale, self.v_coef) if t is not None)


paged._CACHE_TYPES.append(SagePagedRowCache)
