"""A persistent quantized KV cache for the split-KV operators (include/sageattn_hip_kvcache.h holds the rule).

``sageattn_splitkv`` / ``sageattn_splitkv_causal`` run the whole length-aware K / V pre-pass on every call, although a decode
step changes one row of the cache.  ``SageKVCache`` keeps the prepared operands -- INT8 K and its scales, the smoothing vector,
for FP8 P.V the V^T image and its scale -- across calls; ``append`` extends them in place with one launch
(sage_kv_cache_append) and ``sageattn_splitkv_cached`` is the attention launch and the merge on them, with no pre-pass.

The ops live in a namespace of their own, ``torch.ops.sageattention_amd_kvcache``: ``kv_cache_append`` (it mutates the state)
and ``attn_splitkv_cached[_lse]`` / ``attn_splitkv_causal_cached[_lse]``; everything here traces under
``torch.compile(fullgraph=True)`` and captures into a HIP graph (lengths are read on the device only).

Not built: dropping the caller's fp16 K buffer (the ragged tile is quantized again from its fp16 rows; without them the cache
needs a 64-row fp16 tail per head and a sequential walk), moving the frozen mean or V scale without preparing again, V
smoothing and ``smooth_k=False``.  Paged / block-table caches: ``SagePagedKVCache`` (paged.py)."""
from typing import Any, Optional

import torch

from . import _lib as L
from . import core

__all__ = ["SageKVCache", "sageattn_splitkv_cached"]

_NS = "sageattention_amd_kvcache"


# ---- ops ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::kv_cache_append", mutates_args=("k8", "k_scale", "v8"))
def kv_cache_append(k: torch.Tensor, v: Optional[torch.Tensor], km: torch.Tensor, k8: torch.Tensor, k_scale: torch.Tensor,
                    v8: Optional[torch.Tensor], v_coef: Optional[torch.Tensor], start_lens: torch.Tensor,
                    kv_lens: torch.Tensor, max_new: int, tensor_layout: str, qk_quant_gran: str) -> None:
    """sage_kv_cache_append on the tensors of a cache: one launch; ``v8`` None: no V half"""
    B, H, N, D = L.dims(k, tensor_layout)
    gran, rnd = core._k_pairing(qk_quant_gran)
    with torch.cuda.device(k.device):
        L.check(L.lib().sage_kv_cache_append(
            L.desc(k, tensor_layout), None if v8 is None else L.desc(v, tensor_layout), L.dtype_code(k.dtype), B, H, N, D,
            km.data_ptr(), L.desc(k8, tensor_layout), k_scale.data_ptr(), gran, rnd,
            None if v8 is None else L.desc_vt(v8, tensor_layout), L.ptr(v_coef), start_lens.data_ptr(), kv_lens.data_ptr(),
            int(max_new), L.stream_ptr(k.device)), "sage_kv_cache_append")


@kv_cache_append.register_fake
def _(k, v, km, k8, k_scale, v8, v_coef, start_lens, kv_lens, max_new, tensor_layout, qk_quant_gran):
    return None


def _register_attn(name, causal, with_lse):
    """attn_splitkv[_causal]_cached[_lse]: ``core._splitkv_attn`` on prepared operands (``v``: the fp16 / bf16 V buffer, or
    with a ``v_scale`` the FP8 V^T image); num_splits 0 = ``core.splitkv_num_splits``; o is contiguous in q's shape"""
    params = ("Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor? kv_lens, SymInt num_splits, "
              + "SymInt q_fold, " * causal + "str tensor_layout, float sm_scale, str qk_quant_gran")

    def body(q, k8, k_scale, km, v, v_scale, kv_lens, num_splits, *rest):
        q_fold = rest[0] if causal else None
        tensor_layout, sm_scale, qk_quant_gran = rest[-3:]
        B, Hq, M, _ = L.dims(q, tensor_layout)
        num_splits = num_splits or core.splitkv_num_splits(B, Hq, M, L.dims(k8, tensor_layout)[2])
        with torch.cuda.device(q.device):
            q = core._abi_view(q)  # (a view the C ABI cannot address travels as a contiguous copy, as in the operators)
            o, lse = core._splitkv_attn(q, (k8, k_scale, km, v, v_scale, None), tensor_layout, (qk_quant_gran, 32), sm_scale,
                                        with_lse, kv_lens, num_splits, q_fold=q_fold)
        return (o, lse) if with_lse else o

    def fake(q, k8, k_scale, km, v, v_scale, kv_lens, num_splits, *rest):
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


attn_splitkv_cached = _register_attn("attn_splitkv_cached", False, False)
attn_splitkv_cached_lse = _register_attn("attn_splitkv_cached_lse", False, True)
attn_splitkv_causal_cached = _register_attn("attn_splitkv_causal_cached", True, False)
attn_splitkv_causal_cached_lse = _register_attn("attn_splitkv_causal_cached_lse", True, True)


# ---- the cache ----------------------------------------------------------------------------------------------------------------
class SageKVCache:
    """Prepared split-KV operands of a padded ``[B,Hk,N,D]`` (HND; NHD: ``[B,N,Hk,D]``) KV cache that persist across calls.

    ``prepare`` binds the caller's k and v buffers -- the caller goes on writing new rows into them -- and quantizes the first
    ``kv_lens[b]`` rows of every batch; ``append`` brings the state up to date after rows were written.  The rule
    (include/sageattn_hip_kvcache.h):

    * the K smoothing vector ``km`` is frozen at prepare time.  Softmax does not see a vector subtracted from every key and
      the kernels add ``q.km`` back into the LSE, so exactness does not depend on km being the current mean; only
      quantization quality does.
    * after any sequence of appends the INT8 rows below ``len_b`` and their scales equal a from-scratch quantization of
      ``k[b, :len_b]`` against km, bit for bit; rows at and beyond ``len_b`` of k and v are never read.
    * FP8 P.V: the per-channel V scale is frozen too, as ``v_headroom`` times the scale of the prepared prefix.  Later values
      beyond ``v_headroom`` times the prefix maximum of their channel SATURATE to +-448 times the frozen scale (the append
      clamps before the FP8 conversion, which on its own returns NaN beyond the range); choose the headroom (default 2.0) for
      the drift of your data, or prepare again.  FP16 / BF16 P.V keeps no V state.

    State tensors (all lead with B): ``k8``, ``k_scale``, ``km``; FP8: ``v8``, ``v_scale`` (the frozen one), ``v_coef``."""

    def __init__(self, k, v, pv, qk_quant_gran, tensor_layout, v_headroom):
        self.k, self.v, self.pv, self.qk_quant_gran, self.tensor_layout = k, v, pv, qk_quant_gran, tensor_layout
        self.v_headroom = v_headroom
        self.k8 = self.k_scale = self.km = self.v8 = self.v_scale = self.v_coef = None

    @classmethod
    def prepare(cls, k: torch.Tensor, v: torch.Tensor, kv_lens: torch.Tensor, pv: str = "fp16",
                qk_quant_gran: str = "per_thread", tensor_layout: str = "HND", v_headroom: float = 2.0) -> "SageKVCache":
        """Bind k and v and prepare the first ``clamp(kv_lens[b], 0, N)`` rows of every batch: the length-aware pre-pass of
        ``sageattn_splitkv`` (two launches), and for ``pv="fp8"`` the V^T image written again under the frozen scale.
        head_dim must be 64 or 128 and the buffers 16-byte aligned with strides that are multiples of 16 bytes: a padded or
        re-laid-out copy would break the binding."""
        core._check_sparse_args(pv, qk_quant_gran, tensor_layout)
        if isinstance(v_headroom, bool) or not isinstance(v_headroom, (int, float)):
            raise TypeError(f"v_headroom must be a float >= 1, got {type(v_headroom).__name__}")
        if not v_headroom >= 1:
            raise ValueError(f"v_headroom must be >= 1, got {v_headroom}")
        if k.dim() != 4 or v.dim() != 4:
            raise ValueError("k and v must be 4-D")
        if k.size(-1) not in (64, 128) or v.size(-1) != k.size(-1):
            raise ValueError(f"SageKVCache needs head_dim 64 or 128 (no padded copy: the cache binds the buffers), got "
                             f"{k.size(-1)} and {v.size(-1)}")
        if k.dtype not in (torch.float16, torch.bfloat16) or v.dtype != k.dtype or v.device != k.device:
            raise ValueError("k and v must be fp16 or bf16 tensors of one dtype on one device")
        if pv == "fp8" and k.shape != v.shape:
            raise ValueError(f"pv='fp8' needs k and v of one shape, got {tuple(k.shape)} and {tuple(v.shape)}")
        if k.stride(-1) != 1 or v.stride(-1) != 1 or core._abi_view(k) is not k or core._abi_view(v) is not v:
            raise ValueError("k and v must be 16-byte aligned with a contiguous last dim and strides that are multiples of 16 "
                             "bytes: the cache binds the buffers and cannot take a copy")
        cache = cls(k, v, pv, qk_quant_gran, tensor_layout, float(v_headroom))
        cache.prepare_(kv_lens)
        return cache

    def prepare_(self, kv_lens: torch.Tensor) -> "SageKVCache":
        """Prepare again from the bound buffers at these lengths: new frozen statistics.  On a ``narrow``-ed cache this
        re-prepares its batches alone, into the shared storage."""
        kv_lens = core._check_kv_lens(kv_lens, self.k.size(0), self.k.device)
        with torch.cuda.device(self.k.device):
            k8, ks, km, v8, v_scale, _ = core._prepass(self.k, self.v, self.tensor_layout, self.qk_quant_gran, True,
                                                       self.pv == "fp8", False, kv_lens)
            state = {"k8": k8, "k_scale": ks, "km": km}
            if self.pv == "fp8":
                v_scale_c = v_scale * self.v_headroom            # fp32 product
                v_coef = torch.zeros((*v_scale.shape[:2], 2, v_scale.shape[2]), dtype=torch.float32, device=v_scale.device)
                v_coef[:, :, 1] = torch.where(v_scale_c == 0, torch.zeros_like(v_scale_c), 1.0 / v_scale_c)
                state.update(v8=v8, v_scale=v_scale_c, v_coef=v_coef)
            for name, t in state.items():
                if getattr(self, name) is None:
                    setattr(self, name, t)       # the first prepare owns what the pre-pass allocated
                else:
                    getattr(self, name).copy_(t)  # a later one writes into the (possibly shared) storage
            if self.pv == "fp8":  # the V^T image under the frozen coefficients: every block of the prefix
                self.append(torch.zeros_like(kv_lens), kv_lens, L.dims(self.k, self.tensor_layout)[2])
        return self

    def append(self, start_lens: torch.Tensor, kv_lens: torch.Tensor, max_new: int) -> None:
        """Bring the state up to date after the caller wrote rows ``[start_lens[b], kv_lens[b])`` of k and v: ONE launch that
        quantizes the 64-key tiles from the one holding row ``min(start_b, len_b - 1)`` to the last of ``len_b`` rows (both
        lengths int32 [B] on the device, clamped to [0, N], read on the device only).  ``start_b >= len_b`` adds no rows -- or
        follows a rollback of rejected speculative tokens -- and re-quantizes exactly the tile holding row ``len_b - 1``.
        ``max_new`` (host int >= 1) bounds ``len_b - start_b`` over the batches and sizes the grid.  Rows below ``start_b``
        must be unchanged since they were quantized (not checked)."""
        if isinstance(max_new, bool) or not isinstance(max_new, int):
            raise TypeError(f"max_new must be an int >= 1, got {type(max_new).__name__}")
        if max_new < 1:
            raise ValueError(f"max_new must be >= 1, got {max_new}")
        B = self.k.size(0)
        start_lens = core._check_kv_lens(start_lens, B, self.k.device)
        kv_lens = core._check_kv_lens(kv_lens, B, self.k.device)
        fp8 = self.pv == "fp8"
        torch.ops.sageattention_amd_kvcache.kv_cache_append(
            self.k, self.v if fp8 else None, self.km, self.k8, self.k_scale, self.v8, self.v_coef, start_lens, kv_lens,
            max_new, self.tensor_layout, self.qk_quant_gran)

    def narrow(self, b0: int, nb: int) -> "SageKVCache":
        """A cache over the batches ``[b0, b0 + nb)`` that shares storage with this one (every state tensor leads with B):
        ``prepare_`` on it re-prepares a serving slot alone."""
        c = SageKVCache(self.k.narrow(0, b0, nb), self.v.narrow(0, b0, nb), self.pv, self.qk_quant_gran, self.tensor_layout,
                        self.v_headroom)
        for name in ("k8", "k_scale", "km", "v8", "v_scale", "v_coef"):
            t = getattr(self, name)
            setattr(c, name, None if t is None else t.narrow(0, b0, nb))
        return c

    def operands(self):
        """(k8, k_scale, km, v operand, v_scale or None, None): the ``kv`` of ``core._splitkv_attn``"""
        fp8 = self.pv == "fp8"
        return self.k8, self.k_scale, self.km, self.v8 if fp8 else self.v, self.v_scale if fp8 else None, None


def sageattn_splitkv_cached(q: torch.Tensor, cache: SageKVCache, kv_lens: Optional[torch.Tensor] = None,
                            num_splits: Optional[int] = None, causal: bool = False, q_fold: int = 1,
                            sm_scale: Optional[float] = None, return_lse: bool = False, **refused: Any):
    """``sageattn_splitkv`` (``causal=True``: ``sageattn_splitkv_causal`` with ``q_fold``) on the operands of a
    ``SageKVCache``: no pre-pass, the attention launch over the splits and the merge only.  Layout, ``pv`` and
    ``qk_quant_gran`` are the cache's; ``kv_lens`` is what was last appended (None: every batch has N keys, all of which must
    have been appended).  o and lse are bit-identical to ``core._splitkv_attn`` on a from-scratch quantization of the current
    prefix against the cache's frozen statistics, and exact attention in real arithmetic whatever those are.

    ``num_splits``: 1..16, or None for ``splitkv_num_splits(B, Hq, M, N)``; 1 runs the split kernel with one split for both
    forms (handing over to a dense operator would bring the pre-pass back).  q must have the cache's head_dim (64 or 128).
    What the two split-KV operators refuse by name (``is_causal``, ``attn_mask``, ``block_map`` / ``plan``, ``cu_seqlens_q`` /
    ``cu_seqlens_k``, ``smooth_k=False``, ``smooth_v``) is refused here in the same words."""
    if not isinstance(cache, SageKVCache):
        raise TypeError(f"cache must be a SageKVCache, got {type(cache).__name__}")
    if isinstance(causal, torch.Tensor) or not isinstance(causal, (bool, int)):
        raise TypeError(f"causal must be a bool, got {type(causal).__name__}")
    causal = bool(causal)
    op_name = "sageattn_splitkv_causal" if causal else "sageattn_splitkv"
    kv_lens, num_splits, M = core._splitkv_front(op_name, causal, q, cache.k, cache.v, kv_lens, num_splits,
                                                 cache.tensor_layout, cache.pv, cache.qk_quant_gran, refused)
    if isinstance(q_fold, bool) or not isinstance(q_fold, int):
        raise TypeError(f"q_fold must be an int >= 1, got {type(q_fold).__name__}")
    if q_fold < 1 or M % q_fold != 0 or (q_fold != 1 and not causal):
        raise ValueError(f"q_fold must be >= 1 and divide the {M} query rows (and 1 unless causal), got {q_fold}")
    if q.dtype != cache.k.dtype or q.device != cache.k.device:
        raise ValueError("q must have the dtype and device of the cache's k")
    D = cache.k.size(-1)
    if q.size(-1) != D:
        raise ValueError(f"q must have the cache's head_dim {D}, got {q.size(-1)}")
    Hq, Hk = L.dims(q, cache.tensor_layout)[1], L.dims(cache.k, cache.tensor_layout)[1]
    if Hq % Hk != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({Hk})")
    if sm_scale is None:
        sm_scale = D ** -0.5
    k8, ks, km, v, v_scale, _ = cache.operands()
    ns = torch.ops.sageattention_amd_kvcache
    fold = (q_fold,) if causal else ()
    op = getattr(ns, f"attn_splitkv{'_causal' if causal else ''}_cached{'_lse' if return_lse else ''}")
    return op(q, k8, ks, km, v, v_scale, kv_lens, num_splits, *fold, cache.tensor_layout, float(sm_scale),
              cache.qk_quant_gran)
