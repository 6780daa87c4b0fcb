"""An MXFP4 image of V for the persistent quantized KV cache (include/sageattn_hip_fp4.h holds the rule).

Few query rows against a long cache are bound by the bytes of K and V.  ``SageKVCacheV4`` is ``SageKVCache`` with V kept as
FP4 (e2m1) nibbles and one e8m0 scale byte per 32 tokens of a channel -- 64 + 4 bytes per key and KV head at head_dim 128
where the FP8 cache has 128 and the FP16-PV cache 256 -- multiplied by the instruction of the FP8 P.V loop, which takes V^T
as FP4 and P as e4m3.  The scale groups live inside one 64-key tile, like the scale groups of K, so growth is local: nothing
of V is frozen, there is no ``v_headroom``, and later values never saturate against an earlier range.

    img, scale = quant_v_mxfp4(v, kv_lens)                        the image of a tensor, one launch
    cache = SageKVCacheV4.prepare(k, v, kv_lens)                  bind the buffers, quantize the prefix
    cache.append(start_lens, kv_lens, max_new)                    ONE launch: K and the image
    o = sageattn_splitkv_v4(q, cache, kv_lens)                    the attention launch over the splits and the merge

The K half (``k8``, ``k_scale``, the frozen ``km``) is that of ``SageKVCache``, by the same code.  The ops live in
``torch.ops.sageattention_amd_fp4`` (ops.py); everything traces under ``torch.compile(fullgraph=True)`` and captures into a
HIP graph.

The same image for a cache kept in pages: ``SagePagedKVCacheV4`` (paged_fp4.py).

Not built: an FP4 image for ``SagePagedRowCache`` and the shared-prefix operator on the paged FP4 cache; the uncached and dense
operators (their pre-pass reads fp16 V, so no bytes are saved); FP4 / FP6 for P or for Q / K (which would also double the MFMA
rate); V smoothing."""
from typing import Any, Optional

import torch

from . import _lib as L
from . import core
from . import ops  # noqa: F401  (registers torch.ops.sageattention_amd_fp4)
from .kvcache import SageKVCache

__all__ = ["quant_v_mxfp4", "SageKVCacheV4", "sageattn_splitkv_v4"]

_OPS = torch.ops.sageattention_amd_fp4


def _check_v(v, tensor_layout):
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")
    if not isinstance(v, torch.Tensor) or v.dim() != 4:
        raise ValueError("v must be 4-D")
    if v.size(-1) not in (64, 128):
        raise ValueError(f"the MXFP4 V image needs head_dim 64 or 128, got {v.size(-1)}")
    if v.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("v must be an fp16 or bf16 tensor")
    if v.stride(-1) != 1 or core._abi_view(v) is not v:
        raise ValueError("v must be 16-byte aligned with a contiguous last dim and strides that are multiples of 16 bytes")


def _image_shapes(v, tensor_layout):
    B, H, N, D = L.dims(v, tensor_layout)
    T = (N + 63) // 64
    return (B, H, D, 32 * T), (B, H, T, 2 * D)


def _alloc_image(v, tensor_layout):
    """(img, scale) for v: zero nibbles and the scale byte 127 = 2^0 everywhere, so that a tile no call has written yet
    decodes to zeros"""
    si, ss = _image_shapes(v, tensor_layout)
    return torch.zeros(si, dtype=torch.uint8, device=v.device), torch.full(ss, 127, dtype=torch.uint8, device=v.device)


def quant_v_mxfp4(v: torch.Tensor, kv_lens: Optional[torch.Tensor] = None, tensor_layout: str = "HND", out=None):
    """The MXFP4 image of ``v`` ([B,Hk,N,D], NHD: [B,N,Hk,D]; fp16 / bf16, head_dim 64 or 128): ``img`` uint8
    [B,Hk,D,32*ceil(N/64)], two e2m1 nibbles per byte in the MFMA token order, and ``scale`` uint8 [B,Hk,ceil(N/64),2*D], the
    e8m0 bytes of the groups of 32 tokens.  One launch, one pass over v.  With ``kv_lens`` (int32 [B] on the device, read
    there only) batch b has the rows below ``clamp(kv_lens[b], 0, N)``: rows at or beyond are never loaded, and no byte of a
    tile at or beyond ``ceil(len_b / 64)`` is written.  ``out=(img, scale)``: the caller's buffers."""
    _check_v(v, tensor_layout)
    if kv_lens is not None:
        kv_lens = core._check_kv_lens(kv_lens, v.size(0), v.device)
    img, scale = _alloc_image(v, tensor_layout) if out is None else out
    for t, shape, name in zip((img, scale), _image_shapes(v, tensor_layout), ("img", "scale")):
        if t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != v.device:
            raise ValueError(f"{name} must be a contiguous uint8 tensor of shape {shape} on v's device")
    _OPS.quant_v_mxfp4(v, img, scale, kv_lens, tensor_layout)
    return img, scale


class SageKVCacheV4:
    """``SageKVCache`` with V as an MXFP4 image.  ``prepare`` binds the caller's padded k and v buffers and quantizes the first
    ``kv_lens[b]`` rows; ``append`` brings K and the image up to date after rows were written, in one launch.  After any
    sequence of appends the valid tiles of ``v4`` / ``v4_scale`` equal ``quant_v_mxfp4`` of the current prefix and the K state
    what ``SageKVCache.append`` gives, bit for bit; rows at and beyond ``len_b`` of k and v are never read.

    State tensors (all lead with B): ``k8``, ``k_scale``, ``km`` (frozen at prepare time), ``v4``, ``v4_scale``."""

    def __init__(self, kc: SageKVCache, v4, v4_scale):
        self._kc, self.v4, self.v4_scale = kc, v4, v4_scale

    # the K half is a SageKVCache without V state: its buffers, its strings and its tensors are this cache's
    k = property(lambda self: self._kc.k)
    v = property(lambda self: self._kc.v)
    k8 = property(lambda self: self._kc.k8)
    k_scale = property(lambda self: self._kc.k_scale)
    km = property(lambda self: self._kc.km)
    qk_quant_gran = property(lambda self: self._kc.qk_quant_gran)
    tensor_layout = property(lambda self: self._kc.tensor_layout)

    @classmethod
    def prepare(cls, k: torch.Tensor, v: torch.Tensor, kv_lens: torch.Tensor, qk_quant_gran: str = "per_thread",
                tensor_layout: str = "HND") -> "SageKVCacheV4":
        """Bind k and v and prepare the first ``clamp(kv_lens[b], 0, N)`` rows of every batch: the K pre-pass of
        ``SageKVCache.prepare`` (its checks: head_dim 64 or 128, aligned buffers of one dtype) and one launch for the image."""
        kc = SageKVCache.prepare(k, v, kv_lens, "fp16", qk_quant_gran, tensor_layout)
        if k.shape != v.shape:
            raise ValueError(f"SageKVCacheV4 needs k and v of one shape, got {tuple(k.shape)} and {tuple(v.shape)}")
        cache = cls(kc, *_alloc_image(v, tensor_layout))
        _OPS.quant_v_mxfp4(v, cache.v4, cache.v4_scale, core._check_kv_lens(kv_lens, k.size(0), k.device), tensor_layout)
        return cache

    def prepare_(self, kv_lens: torch.Tensor) -> "SageKVCacheV4":
        """Prepare again from the bound buffers at these lengths (a new frozen km); on a ``narrow``-ed cache its batches alone"""
        self._kc.prepare_(kv_lens)
        _OPS.quant_v_mxfp4(self.v, self.v4, self.v4_scale, core._check_kv_lens(kv_lens, self.k.size(0), self.k.device),
                           self.tensor_layout)
        return self

    def append(self, start_lens: torch.Tensor, kv_lens: torch.Tensor, max_new: int) -> None:
        """``SageKVCache.append`` for K and the image: ONE launch that re-quantizes the 64-key tiles from the one holding row
        ``min(start_b, len_b - 1)`` to the last of ``len_b`` rows from the bound rows.  ``start_b >= len_b`` (no new rows, or a
        rollback) re-quantizes exactly the ragged tile; an empty batch touches nothing."""
        if isinstance(max_new, bool) or not isinstance(max_new, int):
            raise TypeError(f"max_new must be an int >= 1, got {type(max_new).__name__}")
        if max_new < 1:
            raise ValueError(f"max_new must be >= 1, got {max_new}")
        B = self.k.size(0)
        start_lens = core._check_kv_lens(start_lens, B, self.k.device)
        kv_lens = core._check_kv_lens(kv_lens, B, self.k.device)
        _OPS.kv_cache_append_v4(self.k, self.v, self.km, self.k8, self.k_scale, self.v4, self.v4_scale, start_lens, kv_lens,
                                max_new, self.tensor_layout, self.qk_quant_gran)

    def narrow(self, b0: int, nb: int) -> "SageKVCacheV4":
        """A cache over the batches ``[b0, b0 + nb)`` that shares storage with this one"""
        return SageKVCacheV4(self._kc.narrow(b0, nb), self.v4.narrow(0, b0, nb), self.v4_scale.narrow(0, b0, nb))


def sageattn_splitkv_v4(q: torch.Tensor, cache: SageKVCacheV4, kv_lens: Optional[torch.Tensor] = None,
                        num_splits: Optional[int] = None, causal: bool = False, q_fold: int = 1,
                        sm_scale: Optional[float] = None, return_lse: bool = False, **refused: Any):
    """``sageattn_splitkv_cached`` on a ``SageKVCacheV4``: the attention launch over the splits -- P.V on the MXFP4 image --
    and the merge.  The split rule, ``kv_lens``, ``num_splits`` (1 runs the split kernel with one split), ``causal`` with its
    bottom-right alignment and ``q_fold`` are those of the cached operator, and so is everything it refuses by name.  lse is
    bit-identical to the lse of the FP8 cache on the same tensors: V does not enter it."""
    if not isinstance(cache, SageKVCacheV4):
        raise TypeError(f"cache must be a SageKVCacheV4, got {type(cache).__name__}")
    if isinstance(causal, torch.Tensor) or not isinstance(causal, (bool, int)):
        raise TypeError(f"causal must be a bool, got {type(causal).__name__}")
    causal = bool(causal)
    op_name = "sageattn_splitkv_causal" if causal else "sageattn_splitkv"
    kv_lens, num_splits, M = core._splitkv_front(op_name, causal, q, cache.k, cache.v, kv_lens, num_splits,
                                                 cache.tensor_layout, "fp8", cache.qk_quant_gran, refused)
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
    fold = (q_fold,) if causal else ()
    op = getattr(_OPS, f"attn_splitkv{'_causal' if causal else ''}_v4{'_lse' if return_lse else ''}")
    return op(q, cache.k8, cache.k_scale, cache.km, cache.v4, cache.v4_scale, kv_lens, num_splits, *fold, cache.tensor_layout,
              float(sm_scale), cache.qk_quant_gran)
