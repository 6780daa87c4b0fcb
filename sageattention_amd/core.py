"""Host-side mirror of ``sageattention/core.py`` (reference) for MI355X / gfx950.

Same public names, arguments, defaults, return values and error behaviour as the reference entry points
(``sageattn`` core.py:80, ``sageattn_qk_int8_pv_fp16_triton`` :161, ``sageattn_qk_int8_pv_fp16_cuda`` :480,
``sageattn_qk_int8_pv_fp8_cuda`` :656, ``sageattn_qk_int8_pv_fp8_cuda_sm90`` :908).  Everything below the
argument handling runs as hand-written HIP through the C ABI (include/sageattn_hip.h): K mean, INT8 quantizers
(with the LSE correction fused), V fp16/fp8 preparation and the fused attention kernel.  No Triton, no
rocWMMA, no debug dumps (the fork's torch.save side effects, core.py:320-352,845-881, are not reproduced)."""
import ctypes
import functools
import warnings
from typing import Any, Optional

import os

import torch

from . import _lib as L
from . import _qattn
from .quant import (_quant, block_pool_sim, k_mean, k_smooth_quant, k_smooth_quant_kvlen, kv_prepare_fp8, kv_prepare_fp8_kvlen,
                    per_channel_fp8, sub_mean)

__all__ = ["sageattn", "sageattn_qk_int8_pv_fp16_cuda", "sageattn_qk_int8_pv_fp16_triton",
           "sageattn_qk_int8_pv_fp8_cuda", "sageattn_qk_int8_pv_fp8_cuda_sm90", "sageattn_varlen",
           "sageattn_block_sparse", "block_sparse_plan", "BlockSparsePlan", "sageattn_sparge", "sparge_plan",
           "sageattn_tile_mass", "plan_recall", "sparge_tune", "SpargeTuning", "sageattn_kvlen",
           "sageattn_tile_mass_kvlen", "plan_recall_kvlen", "sparge_tune_kvlen", "sageattn_splitkv", "splitkv_num_splits",
           "sageattn_splitkv_causal"]


def _common_checks(q, k, v):
    dtype = q.dtype
    assert q.is_cuda, "Input tensors must be on cuda."
    assert dtype in [torch.float16, torch.bfloat16], "Input tensors must be in dtype of torch.float16 or torch.bfloat16"
    assert q.device == k.device == v.device, "All tensors must be on the same device."
    assert q.dtype == k.dtype == v.dtype, "All tensors must have the same dtype."
    return dtype


def _pad_head_dim(q, k, v):
    """core.py:590-601"""
    head_dim_og = q.size(-1)
    if head_dim_og < 64:
        pad = 64 - head_dim_og
    elif 64 < head_dim_og < 128:
        pad = 128 - head_dim_og
    elif head_dim_og > 128:
        raise ValueError(f"Unsupported head_dim: {head_dim_og}")
    else:
        pad = 0
    if pad:
        q = torch.nn.functional.pad(q, (0, pad))
        k = torch.nn.functional.pad(k, (0, pad))
        v = torch.nn.functional.pad(v, (0, pad))
    assert q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1, "Last dim of qkv must be contiguous."
    return _abi_view(q), _abi_view(k), _abi_view(v), head_dim_og


def _abi_view(t):
    """The reference takes any tensor whose last dim is contiguous (core.py:592-601); the C ABI wants a 16-byte aligned
    base and strides that are multiples of 16 bytes (csrc/sage_common.h tensor_ok).  A view that does not meet that --
    ``x[..., 4:68]``, a row stride of D + 4 -- is passed as a contiguous copy; every other tensor as it is."""
    unit = 16 // t.element_size()
    if t.data_ptr() % 16 == 0 and all(s % unit == 0 for s in t.stride()[:-1]):
        return t
    return t.contiguous()


def _quant_qk(q, k, km, tensor_layout, qk_quant_gran, sm_scale, WARPQ, want_lse_corr, Hq, Hk):
    """Quantize Q and K with a given mean (core.py:621-624): the pairing tables below, so tests and tools that need
    pre-quantized operands use exactly what the operators use."""
    gran, rnd = _k_pairing(qk_quant_gran)
    k8, ks, _ = _quant(k, tensor_layout, gran, True, 64, 64, 1.0, rnd, mean=km, dense_heads=True)
    q8, qs, corr = _quant_q(q, km, tensor_layout, qk_quant_gran, sm_scale, WARPQ, want_lse_corr, Hq, Hk)
    return q8, qs, k8, ks, corr


def _finish_lse(lse2, corr, sm_scale):
    """core.py:651: lse / 1.44269504 + lse_correction * sm_scale"""
    out = torch.empty_like(lse2)
    L.check(L.lib().sage_finish_lse(lse2.data_ptr(), L.ptr(corr), float(sm_scale), out.data_ptr(), lse2.numel(),
                                    L.stream_ptr(lse2.device)), "sage_finish_lse")
    return out


_GRAN_CODE = {"per_block": L.GRAN_PER_BLOCK, "per_block_cuda": L.GRAN_PER_BLOCK, "per_warp": L.GRAN_PER_WARP,
              "per_thread": L.GRAN_PER_THREAD}

# Fold the Q quantizer into the attention kernel (sage_attn_fusedq_*): same bits, one launch and one pass over Q less.
# Re-measured end to end in round 3 (tools/fuseq_bench.py, profiles/r03_ab/fuseq_crossover.log), after the prologue learnt
# to issue its tile copies before the Q loads: fused <= separate at every length -- 0.96-0.97 at 2K keys, 0.98-1.00 at 4K,
# 0.993 (fp16 PV) / 0.994 (fp8 PV) at C3, 0.995 / 0.992 at C4; cross-attention with 16K-32K query rows on 256-4096 keys
# (tools/cross_bench.py): 1.00-1.11x faster fused -- so there is no length limit any more (round 2 stopped at 4096 rows).  Default ON since round 2: the rare wrong 32-row wave seen under perturbed
# timing in round 1 was an LDS race in the attention kernel's prologue, fixed by one barrier
# (profiles/r02_race_evidence.md).  SAGEATTN_FUSE_Q=0 selects the stand-alone Q quantizer + kernel path (bit-identical).
FUSE_Q_QUANT = os.environ.get("SAGEATTN_FUSE_Q", "1") == "1"
FUSE_Q_MAX_SEQ = 1 << 30


# quantizer pairings of core.py:295-299,621-624: granularity name -> (K granularity, Q granularity, rounding).
# "per_block" = the Triton quantizer (quant_per_block.py), "per_block_cuda" = csrc/fused (quant.py:23-104, RNE), both with
# sm_scale*log2e folded into Q.
_PAIRING = {"per_block": (L.GRAN_PER_BLOCK, L.GRAN_PER_BLOCK, L.ROUND_TRITON),
            "per_block_cuda": (L.GRAN_PER_BLOCK, L.GRAN_PER_BLOCK, L.ROUND_CUDA),
            "per_warp": (L.GRAN_PER_BLOCK, L.GRAN_PER_WARP, L.ROUND_CUDA),
            "per_thread": (L.GRAN_PER_THREAD, L.GRAN_PER_THREAD, L.ROUND_TRITON)}


def _pairing(qk_quant_gran):
    try:
        return _PAIRING[qk_quant_gran]
    except KeyError:
        raise ValueError(f"Unsupported qk_quant_gran: {qk_quant_gran}") from None


def _k_pairing(qk_quant_gran):
    kg, _, rnd = _pairing(qk_quant_gran)
    return kg, rnd


def _prep_k(k, tensor_layout, qk_quant_gran, smooth_k):
    """``km = k.mean(seq)`` (core.py:612) + the K half of the quantizer pairings of core.py:621-624 -> (k8, ks, km).
    Two passes over K in three launches on purpose: single-pass forms (workgroups of a head exchanging partial sums
    inside one launch; one workgroup per head re-reading out of L2) were built and measured SLOWER on MI355X for every
    shape from 2K keys up (pre-pass) -- K's second read is an L2 / Infinity-Cache hit anyway."""
    gran, rnd = _k_pairing(qk_quant_gran)
    if smooth_k:
        return k_smooth_quant(k, tensor_layout, gran, rnd)
    k8, ks, _ = _quant(k, tensor_layout, gran, True, 64, 64, 1.0, rnd, mean=None, dense_heads=True)
    return k8, ks, None


def _quant_q(q, km, tensor_layout, qk_quant_gran, sm_scale, WARPQ, want_lse_corr, Hq, Hk):
    """Q half of core.py:621-624 (+ the LSE correction q.km of core.py:613-617 in the same pass) -> (q8, qs, corr)."""
    _, gran, rnd = _pairing(qk_quant_gran)
    dot_vec = km if (want_lse_corr and km is not None) else None
    if qk_quant_gran in ("per_block", "per_block_cuda"):  # triton path: sm_scale*log2e folded into Q (quant_per_block.py:84)
        return _quant(q, tensor_layout, gran, False, 128, 128, sm_scale * 1.44269504, rnd, dot_vec=dot_vec,
                      dot_group=Hq // Hk, dense_heads=True)
    return _quant(q, tensor_layout, gran, False, 128, WARPQ, 1.0, rnd, dot_vec=dot_vec, dot_group=Hq // Hk, dense_heads=True)


def _prepass(k, v, tensor_layout, qk_quant_gran, smooth_k, pv_fp8, smooth_v, kv_lens=None):
    """The K pre-pass of the multi-call operators, and for FP8 P.V the V pre-pass -> (k8, ks, km, v or v8, v_scale, vm).  ``km``
    is None without ``smooth_k``, ``v_scale`` None for FP16 P.V (v is passed through), ``vm`` None without ``smooth_v``.
    With ``kv_lens`` (``sageattn_kvlen``: K smoothing on, no V smoothing, for FP8 P.V k and v of one shape) the length-aware
    twins: every statistic over the rows < len_b of a batch only."""
    if kv_lens is not None:
        gran, rnd = _k_pairing(qk_quant_gran)
        if pv_fp8:
            return kv_prepare_fp8_kvlen(k, v, kv_lens, tensor_layout, gran, rnd, scale_max=448.0) + (None,)
        return k_smooth_quant_kvlen(k, kv_lens, tensor_layout, gran, rnd) + (v, None, None)
    # K and V by ONE call (sage_kv_prepare_fp8: it smooths K, does not smooth V and wants V in K's shape).  This is what each
    # caller spelled out before: sageattn_qk_int8_pv_fp8_cuda `smooth_k and not smooth_v and k.shape == v.shape and k.dtype ==
    # v.dtype` (pv_fp8 True; equal dtypes are asserted by _common_checks), sageattn_block_sparse `pv == "fp8" and smooth_k and
    # k.shape == v.shape` (smooth_v False), sageattn_sparge `pv == "fp8" and k.shape == v.shape` (smooth_k True, smooth_v False)
    if pv_fp8 and smooth_k and not smooth_v and k.shape == v.shape:
        gran, rnd = _k_pairing(qk_quant_gran)
        return kv_prepare_fp8(k, v, tensor_layout, gran, rnd, scale_max=448.0) + (None,)
    k8, ks, km = _prep_k(k, tensor_layout, qk_quant_gran, smooth_k)
    if not pv_fp8:
        return k8, ks, km, v, None, None
    return (k8, ks, km) + per_channel_fp8(v, tensor_layout=tensor_layout, scale_max=448.0, smooth_v=smooth_v)


def _fused_attn(q, kv, tensor_layout, is_causal, q_quant, sm_scale, return_lse, sparse=None, kv_lens=None):
    """sage_attn_fusedq_pv_{f16,f8} on the operands ``kv`` of ``_prepass`` (FP8 P.V where it has a v_scale); ``q_quant`` is
    (qk_quant_gran, rows per Q scale group).  With ``sparse`` = (plan, pv_thresh, skipped) their block-sparse twins, and with
    a ``pv_thresh`` (fp32 [Hq]) in it the twins with the P.V skip, which fill ``skipped`` (int32 [B,Hq,ceil(M/128),4] or
    None).  With ``kv_lens`` (int32 [B]) the twins with per-batch key lengths: the dense ones, and with ``sparse`` the
    ``_blocksparse_kvlen`` entry points (a None ``pv_thresh`` travels as NULL: no P.V skip).  -> (o, lse or None)"""
    k8, ks, km, v, v_scale, v_mean = kv
    qk_quant_gran, warpq = q_quant
    B, Hq, M, D = L.dims(q, tensor_layout)
    _, Hk, N, _ = L.dims(k8, tensor_layout)
    if Hq % Hk != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({Hk})")
    o = torch.empty(q.size(), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, Hq, M), dtype=torch.float32, device=q.device) if return_lse else None
    vm = v_mean.to(torch.float32).contiguous() if v_mean is not None else None
    shape = (B, Hq, Hk, M, N, D, int(is_causal), _GRAN_CODE[qk_quant_gran], warpq, float(sm_scale))
    if v_scale is not None:
        args = (L.desc(q, tensor_layout), L.dtype_code(q.dtype), L.desc(k8, tensor_layout), L.desc_vt(v, tensor_layout),
                L.desc(o, tensor_layout), L.dtype_code(o.dtype), ks.data_ptr(), L.ptr(km), v_scale.data_ptr(), L.ptr(vm),
                L.ptr(lse)) + shape
        name = "sage_attn_fusedq_pv_f8"
    else:
        args = (L.desc(q, tensor_layout), L.dtype_code(q.dtype), L.desc(k8, tensor_layout), L.desc(v, tensor_layout),
                L.dtype_code(v.dtype), L.desc(o, tensor_layout), L.dtype_code(o.dtype), ks.data_ptr(), L.ptr(km), L.ptr(vm),
                L.ptr(lse)) + shape
        name = "sage_attn_fusedq_pv_f16"
    if sparse is not None:
        plan, pv_thresh, skipped = sparse
        name += "_blocksparse"
        args += (plan.lists.data_ptr(), plan.lists.numel() * 4)
        if kv_lens is not None:
            name += "_kvlen"
            args += (L.ptr(pv_thresh), L.ptr(skipped), kv_lens.data_ptr())
        elif pv_thresh is not None:
            name += "_pvskip"
            args += (pv_thresh.data_ptr(), L.ptr(skipped))
    elif kv_lens is not None:
        name += "_kvlen"
        args += (kv_lens.data_ptr(),)
    L.check(getattr(L.lib(), name)(*args, L.stream_ptr(q.device)), name)
    return o, lse


# One ctypes crossing and two allocations (output + workspace) per call: sage_sageattn_pv_{f16,f8} (csrc/sage_op.hip)
# sequences the same entry points the multi-call path below uses, bit-identical.  SAGEATTN_ONE_CALL=0 selects that path.
ONE_CALL = os.environ.get("SAGEATTN_ONE_CALL", "1") == "1"


def _one_call(q, k, v, tensor_layout, is_causal, qk_quant_gran, warpq, sm_scale, return_lse, pv_fp8, scale_max=448.0):
    B, Hq, M, D = L.dims(q, tensor_layout)
    _, Hk, N, _ = L.dims(k, tensor_layout)
    if Hq % Hk != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({Hk})")
    lib = L.lib()
    opts = L.OpOpts(_GRAN_CODE[qk_quant_gran], warpq, 1, 1 if (FUSE_Q_QUANT and M <= FUSE_Q_MAX_SEQ) else 0, 0)
    nbytes = lib.sage_sageattn_workspace_bytes(int(pv_fp8), B, Hq, Hk, M, N, D, int(return_lse), opts)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    o = torch.empty(q.size(), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, Hq, M), dtype=torch.float32, device=q.device) if return_lse else None
    code, st = L.dtype_code(q.dtype), L.stream_ptr(q.device)
    qd, kd, vd, od = (L.desc(t, tensor_layout) for t in (q, k, v, o))
    if pv_fp8:
        L.check(lib.sage_sageattn_pv_f8(qd, kd, vd, code, od, L.ptr(lse), B, Hq, Hk, M, N, D, int(is_causal), float(sm_scale),
                                        float(scale_max), opts, ws.data_ptr(), nbytes, st), "sage_sageattn_pv_f8")
    else:
        L.check(lib.sage_sageattn_pv_f16(qd, kd, vd, code, od, L.ptr(lse), B, Hq, Hk, M, N, D, int(is_causal), float(sm_scale),
                                         opts, ws.data_ptr(), nbytes, st), "sage_sageattn_pv_f16")
    return o, lse


def _sage_fp16(q, k, v, tensor_layout, is_causal, qk_quant_gran, sm_scale, smooth_k, smooth_v, return_lse, WARPQ=32):
    dtype = q.dtype
    with torch.cuda.device(q.device):  # the reference's torch.cuda.set_device(v.device) workaround, core.py:583
        q, k, v, head_dim_og = _pad_head_dim(q, k, v)
        if sm_scale is None:
            sm_scale = head_dim_og ** -0.5
        _, Hq, _, _ = L.dims(q, tensor_layout)
        _, Hk, _, _ = L.dims(k, tensor_layout)
        if ONE_CALL and smooth_k and not smooth_v and qk_quant_gran in ("per_warp", "per_thread"):
            o, lse = _one_call(q, k, v, tensor_layout, is_causal, qk_quant_gran, WARPQ, sm_scale, return_lse, False)
            return _pack(o[..., :head_dim_og], lse, None, None)
        k8, ks, km = _prep_k(k, tensor_layout, qk_quant_gran, smooth_k)
        vm = None
        if smooth_v:
            v, vm = sub_mean(v, tensor_layout)
        if FUSE_Q_QUANT and not qk_quant_gran.startswith("per_block") and L.dims(q, tensor_layout)[2] <= FUSE_Q_MAX_SEQ:
            o, lse = _fused_attn(q, (k8, ks, km, v, None, vm), tensor_layout, is_causal, (qk_quant_gran, WARPQ), sm_scale,
                                 return_lse)
            return _pack(o[..., :head_dim_og], lse, None, None)
        o = torch.empty(q.size(), dtype=dtype, device=q.device)
        q8, qs, corr = _quant_q(q, km, tensor_layout, qk_quant_gran, sm_scale, WARPQ, return_lse, Hq, Hk)
        lse2 = _qattn._attn_f16(q8, k8, v, o, qs, ks, vm, 0 if tensor_layout == "NHD" else 1, int(is_causal),
                                _GRAN_CODE[qk_quant_gran], sm_scale, int(return_lse),
                                logit_mult_is_one=qk_quant_gran.startswith("per_block"))
        lse = _finish_lse(lse2, corr if smooth_k else None, sm_scale) if return_lse else None
        return _pack(o[..., :head_dim_og], lse, None, None)


@torch.compiler.disable
def sageattn_qk_int8_pv_fp16_cuda(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    tensor_layout: str = "HND",
    is_causal: bool = False,
    qk_quant_gran: str = "per_thread",
    sm_scale: Optional[float] = None,
    pv_accum_dtype: str = "fp32",
    smooth_k: bool = True,
    smooth_v: bool = False,
    return_lse: bool = False,
    **kwargs: Any,
) -> torch.Tensor:
    """SageAttention with INT8 Q/K and FP16 PV (reference core.py:480-653).

    On gfx950 the PV MFMA (v_mfma_f32_32x32x16_f16) accumulates in fp32 for every ``pv_accum_dtype`` the
    reference names ("fp32", "fp16", "fp16+fp32"); ``smooth_v`` is honoured only for "fp16" as in the reference
    (core.py:628-630) -- it is numerically a no-op with an fp32 accumulator, but kept for API parity.
    Unknown keyword arguments (SDPA's ``attn_mask=``, ``dropout_p=`` ...) are accepted and ignored, as in the
    reference (core.py:492)."""
    _common_checks(q, k, v)
    assert qk_quant_gran in ["per_warp", "per_thread"], "qk_quant_gran must be either 'per_warp' or 'per_thread'."
    if pv_accum_dtype not in ("fp32", "fp16", "fp16+fp32"):
        raise ValueError(f"Unsupported pv_accum_dtype: {pv_accum_dtype}")
    if pv_accum_dtype in ["fp32", "fp16+fp32"] and smooth_v:
        warnings.warn(f"pv_accum_dtype is {pv_accum_dtype}, smooth_v will be ignored.")
        smooth_v = False
    warpq = 16 if (q.size(-1) > 64 and pv_accum_dtype == "fp16+fp32") else 32  # core.py:622
    return _sage_fp16(q, k, v, tensor_layout, is_causal, qk_quant_gran, sm_scale, smooth_k, smooth_v, return_lse, warpq)


@torch.compiler.disable
def sageattn_qk_int8_pv_fp16_triton(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    tensor_layout: str = "HND",
    quantization_backend: str = "triton",
    is_causal: bool = False,
    attn_mask: Optional[torch.Tensor] = None,
    sm_scale: Optional[float] = None,
    smooth_k: bool = True,
    return_lse: bool = False,
    **kwargs: Any,
) -> torch.Tensor:
    """Reference core.py:161-360 (INT8 Q/K, FP16 PV, the reference's Triton kernels), served by the HIP kernels.

    ``quantization_backend`` selects the quantizer pairing the way the fork does (core.py:295-318):
      * ``"triton"``, non-causal (with or without ``attn_mask``): per-thread quantization (quant_per_thread.py) and the
        per-thread kernel (attn_qk_int8_per_thread.py); sm_scale*log2e applied in the kernel.
      * ``"cuda"``: per-block quantization with the CUDA quantizer's rounding (quant.py:23-104, sm_scale*log2e folded
        into Q) and the per-block kernel.
      * causal calls keep the upstream per-block pairing (quant_per_block.py + attn_qk_int8_per_block_causal.py) for
        ``"triton"``: the fork hands per-thread scales to the per-block causal kernel there, which indexes them with
        per-block strides -- not reproduced.
    ``attn_mask`` (bool, or additive in q's dtype; any shape broadcastable to [B,H,M,N]) follows the reference kernels:
    False adds -1e6, an additive mask is added to the base-2 logits (attn_qk_int8_per_thread.py:37-75).  ``sm_scale`` is
    honoured (the fork's per-thread kernel hard-codes 1/sqrt(padded head_dim), attn_qk_int8_per_thread.py:66)."""
    dtype = _common_checks(q, k, v)
    if quantization_backend not in ("triton", "cuda"):
        raise ValueError(f"Unsupported quantization backend: {quantization_backend}")
    if quantization_backend == "cuda":
        gran = "per_block_cuda"
    else:
        gran = "per_block" if is_causal else "per_thread"
    if attn_mask is None:
        return _sage_fp16(q, k, v, tensor_layout, is_causal, gran, sm_scale, smooth_k, False, return_lse)
    # ---- attn_mask (core.py:249-251, 302-318)
    assert attn_mask.dtype == torch.bool or attn_mask.dtype == q.dtype, "attn_mask must be of dtype bool or the same dtype as q."
    assert attn_mask.device == q.device, "All tensors must be on the same device."
    assert not is_causal, "Mask should be None for causal attention."
    with torch.cuda.device(q.device):
        q, k, v, head_dim_og = _pad_head_dim(q, k, v)
        if sm_scale is None:
            sm_scale = 1.0 / (head_dim_og ** 0.5)
        B, Hq, M, D = L.dims(q, tensor_layout)
        _, Hk, N, _ = L.dims(k, tensor_layout)
        try:
            attn_mask = attn_mask.expand((B, Hq, M, N))
        except Exception:
            raise AssertionError(f"attn_mask shape {attn_mask.shape} cannot be broadcast to {(B, Hq, M, N)}")
        # (the reference converts a bf16 V to fp16 here, core.py:289-290; this kernel multiplies it as bf16)
        k8, ks, km = _prep_k(k, tensor_layout, gran, smooth_k)
        q8, qs, corr = _quant_q(q, km, tensor_layout, gran, sm_scale, 32, return_lse, Hq, Hk)
        o = torch.empty(q.size(), dtype=dtype, device=q.device)
        lse2 = torch.empty((B, Hq, M), dtype=torch.float32, device=q.device) if return_lse else None
        kind = 1 if attn_mask.dtype == torch.bool else (2 if attn_mask.dtype == torch.float16 else 3)
        strides = (ctypes.c_int64 * 4)(*attn_mask.stride())
        per_block = gran != "per_thread"
        L.check(L.lib().sage_attn_qk_int8_pv_f16_masked(
            L.desc(q8, tensor_layout), L.desc(k8, tensor_layout), L.desc(v, tensor_layout), L.dtype_code(v.dtype),
            L.desc(o, tensor_layout), L.dtype_code(dtype), qs.data_ptr(), ks.data_ptr(), attn_mask.data_ptr(), kind, strides,
            L.ptr(lse2), B, Hq, Hk, M, N, D, _GRAN_CODE[gran], 128, 128 if per_block else 32, float(sm_scale),
            1 if per_block else 0, L.stream_ptr(q.device)), "sage_attn_qk_int8_pv_f16_masked")
        lse = _finish_lse(lse2, corr if smooth_k else None, sm_scale) if return_lse else None
        return _pack(o[..., :head_dim_og], lse, None, None)


@torch.compiler.disable
def sageattn_qk_int8_pv_fp8_cuda(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    tensor_layout: str = "HND",
    is_causal: bool = False,
    qk_quant_gran: str = "per_thread",
    sm_scale: Optional[float] = None,
    pv_accum_dtype: str = "fp32+fp16",
    smooth_k: bool = True,
    smooth_v: bool = False,
    return_lse: bool = False,
    **kwargs: Any,
) -> torch.Tensor:
    """SageAttention with INT8 Q/K and FP8 (OCP e4m3fn) PV, fp32 accumulation (reference core.py:656-905).
    All of "fp32", "fp32+fp32", "fp32+fp16" accumulate in true fp32 on MFMA (no fp22 accumulator issue, so no
    two-level buffer); V is quantized per channel with scale_max 448 (quant.py:228)."""
    dtype = _common_checks(q, k, v)
    assert qk_quant_gran in ["per_warp", "per_thread"], "qk_quant_gran must be either 'per_warp' or 'per_thread'."
    if pv_accum_dtype not in ("fp32", "fp32+fp32", "fp32+fp16"):
        raise ValueError(f"Unsupported pv_accum_dtype: {pv_accum_dtype}")
    if pv_accum_dtype in ("fp32+fp32", "fp32+fp16") and smooth_v:
        warnings.warn(f"pv_accum_dtype is '{pv_accum_dtype}', smooth_v will be ignored.")
        smooth_v = False
    with torch.cuda.device(q.device):
        q, k, v, head_dim_og = _pad_head_dim(q, k, v)
        if sm_scale is None:
            sm_scale = head_dim_og ** -0.5
        _, Hq, _, _ = L.dims(q, tensor_layout)
        _, Hk, _, _ = L.dims(k, tensor_layout)
        if ONE_CALL and smooth_k and not smooth_v and k.shape == v.shape:
            o, lse = _one_call(q, k, v, tensor_layout, is_causal, qk_quant_gran, 32, sm_scale, return_lse, True)
            return _pack(o[..., :head_dim_og], lse, None, None)
        kv = _prepass(k, v, tensor_layout, qk_quant_gran, smooth_k, True, smooth_v)
        if FUSE_Q_QUANT and L.dims(q, tensor_layout)[2] <= FUSE_Q_MAX_SEQ:
            o, lse = _fused_attn(q, kv, tensor_layout, is_causal, (qk_quant_gran, 32), sm_scale, return_lse)
            return _pack(o[..., :head_dim_og], lse, None, None)
        k8, ks, km, v8, v_scale, vm = kv
        o = torch.empty(q.size(), dtype=dtype, device=q.device)
        q8, qs, corr = _quant_q(q, km, tensor_layout, qk_quant_gran, sm_scale, 32, return_lse, Hq, Hk)
        lse2 = _qattn._attn_f8(q8, k8, v8, o, qs, ks, v_scale, vm, 0 if tensor_layout == "NHD" else 1, int(is_causal),
                               _GRAN_CODE[qk_quant_gran], sm_scale, int(return_lse))
        lse = _finish_lse(lse2, corr if smooth_k else None, sm_scale) if return_lse else None
        return _pack(o[..., :head_dim_og], lse, None, None)


@torch.compiler.disable
def sageattn_qk_int8_pv_fp8_cuda_sm90(q, k, v, tensor_layout="HND", is_causal=False, qk_quant_gran="per_thread",
                                      sm_scale=None, pv_accum_dtype="fp32+fp32", smooth_k=True, return_lse=False,
                                      **kwargs):
    """Reference core.py:908-1065 (Hopper TMA/wgmma variant).  Same operator; served by the gfx950 FP8 kernel."""
    return sageattn_qk_int8_pv_fp8_cuda(q, k, v, tensor_layout=tensor_layout, is_causal=is_causal,
                                        qk_quant_gran=qk_quant_gran, sm_scale=sm_scale, pv_accum_dtype=pv_accum_dtype,
                                        smooth_k=smooth_k, smooth_v=False, return_lse=return_lse)


def dispatch_pv(q: torch.Tensor, k: torch.Tensor, tensor_layout: str = "HND", is_causal: bool = False,
                n_kv: Optional[int] = None) -> str:
    """"fp8" or "fp16": the P.V precision ``sageattn`` uses for these shapes (see its docstring).  ``n_kv`` overrides
    the key count (sequence-parallel callers pass the length of the WHOLE sequence)."""
    choice = os.environ.get("SAGEATTN_DISPATCH", "auto")
    if choice not in ("auto", "fp8", "fp16"):
        raise ValueError(f"SAGEATTN_DISPATCH must be auto, fp8 or fp16, got {choice}")
    if choice != "auto":
        return choice
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")
    if n_kv is None:
        n_kv = k.size(2) if tensor_layout == "HND" else k.size(1)
    keys_per_row = n_kv // 2 if is_causal else n_kv
    return "fp8" if keys_per_row >= (4096 if q.size(-1) <= 64 else 2048) else "fp16"


def sageattn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tensor_layout: str = "HND", is_causal: bool = False,
             sm_scale: Optional[float] = None, return_lse: bool = False, **kwargs: Any):
    """Drop-in for ``F.scaled_dot_product_attention`` (reference core.py:80-144: "automatically selects the optimal
    kernel").  The fork dispatches to the INT8-QK / FP8-PV path with fp32 accumulation (core.py:144), and upstream picks
    its FP8 kernels on every FP8-capable architecture (core.py:151-156): on gfx950 the MX-scaled FP8 MFMA makes that the
    fastest variant from a few thousand keys upwards.  Below that the per-channel V quantizer (two more launches and
    two passes over V) costs more than the FP8 MFMA saves, so short sequences take the FP16-PV operator, which is also
    the more accurate of the two; the crossover was measured end to end (profiles/r01d_sweep_end_to_end.md):
    keys per query row >= 4096 at head_dim <= 64, >= 2048 above (a causal row sees half the keys on average).
    ``SAGEATTN_DISPATCH=fp8|fp16`` pins the choice; the two operators are also exported by name."""
    choice = dispatch_pv(q, k, tensor_layout, is_causal)
    if choice == "fp16":
        return sageattn_qk_int8_pv_fp16_cuda(q, k, v, tensor_layout=tensor_layout, is_causal=is_causal,
                                             sm_scale=sm_scale, return_lse=return_lse, pv_accum_dtype="fp32")
    return sageattn_qk_int8_pv_fp8_cuda(q, k, v, tensor_layout=tensor_layout, is_causal=is_causal, sm_scale=sm_scale,
                                        return_lse=return_lse, pv_accum_dtype="fp32")


@torch.compiler.disable
def sageattn_varlen(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    cu_seqlens_k: torch.Tensor,
    max_seqlen_q: int,
    max_seqlen_k: int,
    is_causal: bool = False,
    sm_scale: Optional[float] = None,
    smooth_k: bool = True,
    **kwargs: Any,
) -> torch.Tensor:
    """Packed variable-length SageAttention (reference core.py:363-477): q ``[cu_seqlens_q[-1], Hq, D]``, k/v
    ``[cu_seqlens_k[-1], Hk, D]``; per-block INT8 Q/K (blocks restart at each sequence), FP16 PV; the K smoothing
    mean is taken over ALL packed tokens (core.py:461).  The cumulative lengths stay on the device: no host sync.

    ``max_seqlen_q`` / ``max_seqlen_k`` may be upper bounds of the true maxima (a serving bucket size): they size the scale
    arrays and the grid and feed the workgroup-geometry choice, and the output has the bits of the call with the exact maxima.
    ``is_causal`` masks top-left PER SEQUENCE: query row i of a sequence sees its keys 0..i, whatever the two lengths are (a
    sequence with more queries than keys shows all its keys to the rows beyond them).  A sequence with queries and no keys
    gives zero rows."""
    dtype = _common_checks(q, k, v)
    assert cu_seqlens_q.is_contiguous() and cu_seqlens_k.is_contiguous(), "cu_seqlens_q and cu_seqlens_k must be contiguous."
    assert q.dim() == 3 and k.dim() == 3 and v.dim() == 3, "q, k, v must be [total_tokens, heads, head_dim]"
    with torch.cuda.device(q.device):
        q, k, v, head_dim_og = _pad_head_dim(q, k, v)
        if sm_scale is None:
            sm_scale = 1.0 / (head_dim_og ** 0.5)
        Tq, Hq, D = q.shape
        Tk, Hk, _ = k.shape
        nseq = cu_seqlens_q.numel() - 1
        cu_q = cu_seqlens_q.to(device=q.device, dtype=torch.int32)
        cu_k = cu_seqlens_k.to(device=q.device, dtype=torch.int32)
        lib, st = L.lib(), L.stream_ptr(q.device)
        code = L.dtype_code(dtype)
        # packed [T,H,D] == NHD with batch 1
        km = k_mean(k.unsqueeze(0), "NHD") if smooth_k else None  # [1,Hk,D]

        def desc3(t):
            return L.SageTensor(t.data_ptr(), 0, t.stride(1), t.stride(0))
        q8 = torch.empty(q.shape, dtype=torch.int8, device=q.device)
        k8 = torch.empty(k.shape, dtype=torch.int8, device=q.device)
        qs = torch.empty((nseq, Hq, (max_seqlen_q + 127) // 128), dtype=torch.float32, device=q.device)
        ks = torch.empty((nseq, Hk, (max_seqlen_k + 63) // 64), dtype=torch.float32, device=q.device)
        L.check(lib.sage_quant_qk_int8_varlen(desc3(q), code, cu_q.data_ptr(), nseq, Hq, int(max_seqlen_q), D, None,
                                              desc3(q8), qs.data_ptr(), L.GRAN_PER_BLOCK, 0, 128, 128,
                                              float(sm_scale * 1.44269504), L.ROUND_TRITON, st), "sage_quant_qk_int8_varlen")
        L.check(lib.sage_quant_qk_int8_varlen(desc3(k), code, cu_k.data_ptr(), nseq, Hk, int(max_seqlen_k), D, L.ptr(km),
                                              desc3(k8), ks.data_ptr(), L.GRAN_PER_BLOCK, 1, 64, 64, 1.0, L.ROUND_TRITON, st),
                "sage_quant_qk_int8_varlen")
        o = torch.empty(q.shape, dtype=dtype, device=q.device)
        L.check(lib.sage_attn_qk_int8_pv_f16_varlen(desc3(q8), desc3(k8), desc3(v), code, desc3(o), code, qs.data_ptr(),
                                                    ks.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), nseq, Hq, Hk,
                                                    int(max_seqlen_q), int(max_seqlen_k), D, int(is_causal), L.GRAN_PER_BLOCK,
                                                    128, 128, float(sm_scale), 1, st), "sage_attn_qk_int8_pv_f16_varlen")
        return o[..., :head_dim_og]


# ---- per-batch key lengths -------------------------------------------------------------------------------------------------
def _check_kv_lens(kv_lens, B, device):
    """``kv_lens`` as the kernels read it: an int32 [B] tensor on q's device (its values stay on the device)"""
    if not isinstance(kv_lens, torch.Tensor):
        raise TypeError("kv_lens must be an int32 tensor of shape [B]")
    if kv_lens.dtype != torch.int32:
        raise TypeError(f"kv_lens must be of dtype int32, got {kv_lens.dtype}")
    if tuple(kv_lens.shape) != (B,):
        raise ValueError(f"kv_lens shape {tuple(kv_lens.shape)} does not match [B={B}]")
    if kv_lens.device != device:
        raise ValueError(f"kv_lens is on {kv_lens.device}, q on {device}")
    return kv_lens.contiguous()


@torch.compiler.disable
def sageattn_kvlen(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    kv_lens: torch.Tensor,
    tensor_layout: str = "HND",
    is_causal: bool = False,
    sm_scale: Optional[float] = None,
    pv: str = "fp16",
    qk_quant_gran: str = "per_thread",
    return_lse: bool = False,
):
    """SageAttention on the ordinary padded layout with a per-batch number of valid keys: batch b attends its keys
    [0, len_b), ``len_b = clamp(kv_lens[b], 0, N)``; ``kv_lens`` is an int32 [B] tensor on q's device, read on the device
    only (no host synchronisation; the call captures into a HIP graph and a replay reads the lengths the tensor holds then).

    For every b with len_b > 0, ``o[b]`` (and ``lse[b]``) are bit-identical to ``sageattn_qk_int8_pv_{fp16,fp8}_cuda`` -- by
    ``pv`` ("fp16" | "fp8", explicit) -- called on ``q[b:b+1]`` and the first len_b keys of ``k[b:b+1]``, ``v[b:b+1]`` with the
    same ``qk_quant_gran``.  Nothing in rows >= len_b of k or v influences any output, NaN and Inf included: the K smoothing
    mean, the K scales and the FP8 V scale are taken over the valid rows only, and the kernel neither copies nor multiplies
    tiles beyond them.  A batch without keys gives o = 0, lse = -inf.  ``is_causal`` is top-left aligned as in the dense
    operator.  K smoothing is always on, V is not smoothed; ``pv="fp8"`` wants k and v of one shape.  The rule:
    include/sageattn_hip.h, per-batch key lengths."""
    _check_sparse_args(pv, qk_quant_gran, tensor_layout)
    kv_lens = _check_kv_lens(kv_lens, q.size(0), q.device)
    if pv == "fp8" and k.shape != v.shape:
        raise ValueError(f"pv='fp8' needs k and v of one shape, got {tuple(k.shape)} and {tuple(v.shape)}")
    _common_checks(q, k, v)
    with torch.cuda.device(q.device):
        q, k, v, head_dim_og = _pad_head_dim(q, k, v)
        if sm_scale is None:
            sm_scale = head_dim_og ** -0.5
        kv = _prepass(k, v, tensor_layout, qk_quant_gran, True, pv == "fp8", False, kv_lens)
        o, lse = _fused_attn(q, kv, tensor_layout, is_causal, (qk_quant_gran, 32), sm_scale, return_lse, kv_lens=kv_lens)
        return _pack(o[..., :head_dim_og], lse, None, None)


# ---- split-KV attention ----------------------------------------------------------------------------------------------------
SPLITKV_MAX = 16               # SAGE_MERGE_MAX (include/sageattn_hip.h)
SPLITKV_MIN_TILES = 8          # key tiles (of 64) a split should keep
SPLITKV_SLOTS = 2 * 256        # resident 4-wave workgroups of an MI355X: two per CU, 256 CUs


def splitkv_num_splits(B: int, Hq: int, M: int, N: int) -> int:
    """The number of splits ``sageattn_splitkv(num_splits=None)`` takes for a call of this shape: from the shape alone (no
    host synchronisation; ``kv_lens`` does not enter),

        min(16, ceil(ntk / 8), ceil(2 * 256 / (B * Hq * ceil(M / 128)))), at least 1,      ntk = ceil(N / 64).

    The third term asks for just enough splits that the grid ``B * Hq * ceil(M/128) * S`` reaches the 512 workgroups an MI355X
    holds at once (two 4-wave workgroups on each of 256 CUs); the second keeps at least 8 key tiles per split, so that the
    prologue, the epilogue and the merge of a split stay small beside its loop; the first is the merge kernel's slot count.
    A grid that fills the chip already resolves to 1.  The two constants (8 tiles per split, two workgroups per CU) were
    counted from the kernel's geometry and then measured (tools/splitkv_bench.py, profiles/splitkv.md: whole calls against the
    dense operator, S swept over {1, 2, 4, 8, 16}); they stood: wherever the rule picks S > 1 the call is faster than the
    dense one by far more than the dense call's spread against itself -- 0.66-0.68x its time at (1, 40, 512, 32760, 128) with
    S = 4, 0.33x (FP16 PV) / 0.46x (FP8 PV) at (1, 32, 128, 65536, 128) with S = 16, 0.49x / 0.77x for a decode step
    (8, 32, 1, 8192, 128) folded by its GQA group with S = 8 -- and within 6 % of the fastest S of the sweep; at
    (4, 32, 8192, 8192, 128) it resolves to 1 (S = 2 there: 1.13-1.16x the dense time)."""
    ntk = (int(N) + 63) // 64
    grid = int(B) * int(Hq) * ((int(M) + 127) // 128)
    return max(1, min(SPLITKV_MAX, -(-ntk // SPLITKV_MIN_TILES), -(-SPLITKV_SLOTS // max(grid, 1))))


def _splitkv_attn(q, kv, tensor_layout, q_quant, sm_scale, return_lse, kv_lens, num_splits, workspace=None, out=None,
                  q_fold=None):
    """sage_attn_fusedq_pv_{f16,f8}_splitkv on the operands ``kv`` of ``_prepass``: the workspace (the fp32 partial results of
    the splits), the attention launch over the splits and the merge.  ``workspace`` (uint8, on q's device) and ``out`` (a
    tensor or view of q's shape and dtype with a contiguous last dim) are the caller's where given: afterwards the workspace
    holds the partials, [S,B,Hq,M,D] fp32 and behind them [S,B,Hq,M] fp32.  With ``q_fold`` (an int): the causal entry points
    sage_attn_fusedq_pv_{f16,f8}_splitkv_causal.  -> (o, lse or None)"""
    k8, ks, km, v, v_scale, _ = kv
    qk_quant_gran, warpq = q_quant
    B, Hq, M, D = L.dims(q, tensor_layout)
    _, Hk, N, _ = L.dims(k8, tensor_layout)
    if Hq % Hk != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({Hk})")
    lib = L.lib()
    o = torch.empty(q.size(), dtype=q.dtype, device=q.device) if out is None else out
    lse = torch.empty((B, Hq, M), dtype=torch.float32, device=q.device) if return_lse else None
    nbytes = lib.sage_splitkv_workspace_bytes(B, Hq, M, D, num_splits)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if workspace is None else workspace
    pv_fp8, causal = v_scale is not None, q_fold is not None
    name = f"sage_attn_fusedq_pv_{'f8' if pv_fp8 else 'f16'}_splitkv{'_causal' if causal else ''}"
    # in the order of the C signatures: the f8 forms have no v_dtype and take v_scale, the causal forms q_fold
    v_args = (L.desc_vt(v, tensor_layout),) if pv_fp8 else (L.desc(v, tensor_layout), L.dtype_code(v.dtype))
    v_scale_args = (v_scale.data_ptr(),) if pv_fp8 else ()
    causal_args = (int(q_fold),) if causal else ()
    L.check(getattr(lib, name)(
        L.desc(q, tensor_layout), L.dtype_code(q.dtype), L.desc(k8, tensor_layout), *v_args, L.desc(o, tensor_layout),
        L.dtype_code(o.dtype), ks.data_ptr(), km.data_ptr(), *v_scale_args, None, L.ptr(lse),
        B, Hq, Hk, M, N, D, _GRAN_CODE[qk_quant_gran], warpq, float(sm_scale),
        L.ptr(kv_lens), num_splits, *causal_args, ws.data_ptr(), ws.numel(), L.stream_ptr(q.device)), name)
    return o, lse


def _splitkv_front(op, causal, q, k, v, kv_lens, num_splits, tensor_layout, pv, qk_quant_gran, refused):
    """The argument handling that ``sageattn_splitkv`` and ``sageattn_splitkv_causal`` (``op``: the name in the messages)
    share: the keywords refused by name -- ``is_causal`` asks for nothing where it is ``causal`` --, the strings, ``kv_lens``,
    ``num_splits`` and the shape.  -> (kv_lens, num_splits resolved, M)"""
    neutral = {"is_causal": causal, "attn_mask": None, "block_map": None, "plan": None, "cu_seqlens_q": None, "cu_seqlens_k": None,
               "smooth_k": True, "smooth_v": False}  # what is not built, and the one value of each that asks for nothing
    for name, value in refused.items():
        if name not in neutral:
            raise TypeError(f"{op}() got an unexpected keyword argument '{name}'")
        if value is not neutral[name]:
            raise ValueError(f"{op} does not take {name}={value!r}: it is {'causal' if causal else 'non-causal'}, without a "
                             "mask, a block map or packed sequences, K smoothing always on and V not smoothed")
    _check_sparse_args(pv, qk_quant_gran, tensor_layout)
    if kv_lens is not None:
        kv_lens = _check_kv_lens(kv_lens, q.size(0), q.device)
        if pv == "fp8" and k.shape != v.shape:
            raise ValueError(f"pv='fp8' with kv_lens needs k and v of one shape, got {tuple(k.shape)} and {tuple(v.shape)}")
    if num_splits is not None:
        if isinstance(num_splits, bool) or not isinstance(num_splits, int):
            raise TypeError(f"num_splits must be an int in [1, {SPLITKV_MAX}] or None, got {type(num_splits).__name__}")
        if not 1 <= num_splits <= SPLITKV_MAX:
            raise ValueError(f"num_splits must be in [1, {SPLITKV_MAX}] (or None: from the shape), got {num_splits}")
    B, Hq, M, _ = L.dims(q, tensor_layout)
    N = L.dims(k, tensor_layout)[2]
    if num_splits is None:
        num_splits = splitkv_num_splits(B, Hq, M, N)
    return kv_lens, num_splits, M


def _splitkv_run(q, k, v, kv_lens, num_splits, tensor_layout, sm_scale, pv, qk_quant_gran, return_lse, q_fold=None):
    """The tail the two split-KV operators share: head-dim padding, the length-aware pre-pass, ``_splitkv_attn``, packing"""
    _common_checks(q, k, v)
    with torch.cuda.device(q.device):
        q, k, v, head_dim_og = _pad_head_dim(q, k, v)
        if sm_scale is None:
            sm_scale = head_dim_og ** -0.5
        kv = _prepass(k, v, tensor_layout, qk_quant_gran, True, pv == "fp8", False, kv_lens)
        o, lse = _splitkv_attn(q, kv, tensor_layout, (qk_quant_gran, 32), sm_scale, return_lse, kv_lens, num_splits,
                               q_fold=q_fold)
        return _pack(o[..., :head_dim_og], lse, None, None)


@torch.compiler.disable
def sageattn_splitkv(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    kv_lens: Optional[torch.Tensor] = None,
    num_splits: Optional[int] = None,
    tensor_layout: str = "HND",
    sm_scale: Optional[float] = None,
    pv: str = "fp16",
    qk_quant_gran: str = "per_thread",
    return_lse: bool = False,
    **refused: Any,
):
    """SageAttention for few query rows against many keys: the key tiles of every (batch, head, 128-row q-block) are spread
    over ``num_splits`` workgroups, each of which runs the ordinary attention loop over its range and stores an fp32 partial
    result, and a second launch merges the partials (log-sum-exp, in split order: deterministic, no atomics) and rounds once
    to the output dtype.  The other operators launch ``B * Hq * ceil(M/128)`` workgroups, which fills an MI355X only with
    many query rows; this one is for text or latent queries over a long video context, a decode step or a speculative chunk
    over a padded KV cache (M = 1..1024, N = 16K..128K).  Nothing dispatches to it implicitly.

    ``kv_lens`` (optional, int32 [B] on q's device, read on the device only: no host synchronisation, the call captures into a
    HIP graph and a replay reads the lengths the tensor holds then) gives batch b its keys [0, len_b), ``len_b =
    clamp(kv_lens[b], 0, N)``, with the statistics of ``sageattn_kvlen``: nothing in rows >= len_b of k or v influences any
    output, NaN and Inf included; a batch without keys gives o = 0, lse = -inf.  Split s of a batch with ``ntk_b =
    ceil(len_b/64)`` tiles owns the tiles ``[s * tps_b, min((s+1) * tps_b, ntk_b))``, ``tps_b = ceil(ntk_b / num_splits)``; the K
    smoothing mean, the K scales and the FP8 V scale are those of the whole call.  The rule: include/sageattn_hip.h, split-KV
    attention.

    ``num_splits``: 1..16, or None for ``splitkv_num_splits(B, Hq, M, N)`` (from the shape only).  A resolved count of 1
    makes exactly the launches of ``sageattn_kvlen`` (with ``kv_lens``) or ``sageattn_qk_int8_pv_{fp16,fp8}_cuda`` (without)
    and returns their bits.  ``pv`` ("fp16" | "fp8") is explicit; ``pv="fp8"`` with ``kv_lens`` wants k and v of one shape.

    Non-causal, K smoothing always on, V not smoothed, ``per_warp`` or ``per_thread`` scales.  ``is_causal``, ``attn_mask``,
    ``block_map`` / ``plan``, ``cu_seqlens_q`` / ``cu_seqlens_k``, ``smooth_k=False`` and ``smooth_v`` are refused by name
    (ValueError): the library's causal mask is top-left aligned, and with M << N it would mask nearly every key.

    Decode with grouped-query attention: with M = 1 a q-block holds one row of 128.  The operator is non-causal, so the
    ``g = Hq // Hk`` query heads of a KV head may be folded into query rows first -- ``q.view(B, Hk, g, D)`` for a
    ``[B, Hq, 1, D]`` query (HND) against the unchanged ``[B, Hk, N, D]`` cache, and ``o.view(B, Hq, 1, D)`` afterwards: K and V
    are then read once per KV head instead of once per query head."""
    kv_lens, num_splits, _ = _splitkv_front("sageattn_splitkv", False, q, k, v, kv_lens, num_splits, tensor_layout, pv,
                                            qk_quant_gran, refused)
    if num_splits == 1:  # the operator this call names: its launches, its bits
        if kv_lens is not None:
            return sageattn_kvlen(q, k, v, kv_lens, tensor_layout=tensor_layout, sm_scale=sm_scale, pv=pv,
                                  qk_quant_gran=qk_quant_gran, return_lse=return_lse)
        dense = sageattn_qk_int8_pv_fp8_cuda if pv == "fp8" else sageattn_qk_int8_pv_fp16_cuda
        return dense(q, k, v, tensor_layout=tensor_layout, is_causal=False, qk_quant_gran=qk_quant_gran, sm_scale=sm_scale,
                     return_lse=return_lse)
    return _splitkv_run(q, k, v, kv_lens, num_splits, tensor_layout, sm_scale, pv, qk_quant_gran, return_lse)


@torch.compiler.disable
def sageattn_splitkv_causal(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    kv_lens: Optional[torch.Tensor] = None,
    num_splits: Optional[int] = None,
    q_fold: int = 1,
    tensor_layout: str = "HND",
    sm_scale: Optional[float] = None,
    pv: str = "fp16",
    qk_quant_gran: str = "per_thread",
    return_lse: bool = False,
    **refused: Any,
):
    """Causal ``sageattn_splitkv`` for a chunk of new tokens at the END of a padded KV cache: a speculative chunk, a
    multi-token decode step, a chunk of a chunked prefill.  The query rows are the last tokens of batch b's ``len_b =
    clamp(kv_lens[b], 0, N)`` valid keys (N without ``kv_lens``) -- the alignment FlashAttention calls bottom-right, where the
    ``is_causal`` of the other operators is top-left aligned.  The rule (include/sageattn_hip.h, causal split-KV attention):

    * ``g = q_fold >= 1`` divides the M query rows: they are ``T = M / g`` tokens, and row r is token ``t = r // g``.
    * ``off_b = len_b - T`` (it may be negative).  Row r attends the keys ``0 <= j <= t + off_b`` and nothing later.
    * A row with ``t + off_b < 0`` has no key -- the chunk is longer than the cache holds -- and gets o = 0, lse = -inf, as
      does every row of a batch with ``len_b = 0``.
    * Split ranges, the statistics of the whole call (K smoothing mean, K scales and FP8 V scale from the length-aware
      pre-pass: nothing in rows >= len_b of k or v influences any output, NaN included) and the deterministic merge in split
      order are those of ``sageattn_splitkv``.  A (batch, head, 128-row q-block, split) none of whose rows has a key in the
      split launches a workgroup that returns at once; the merge derives the same count and does not read its slot.

    The fold is for grouped-query attention: the ``g = Hq // Hk`` query heads of a KV head become query rows, TOKEN-MAJOR --
    ``[B, Hq, T, D] -> [B, Hk, T*g, D]`` (HND), row ``t*g + i`` is head i of token t, i.e. ``q.view(B, Hk, g, T,
    D).transpose(2, 3).reshape(B, Hk, T*g, D)`` and the inverse on o -- so that K and V are read once per KV head and 4
    speculative tokens of 8 heads fill one wave.  All g rows of a token see the same keys.

    ``kv_lens`` (optional int32 [B] on q's device) is read on the device only: no host synchronisation, the call captures into
    a HIP graph and a replay moves the diagonal with the lengths the tensor holds then.  ``num_splits``: 1..16, or None for
    ``splitkv_num_splits(B, Hq, M, N)``; 1 is valid and runs the same kernel with one split (there is no dense operator with
    this alignment to hand over to).  ``pv`` ("fp16" | "fp8") is explicit; ``pv="fp8"`` with ``kv_lens`` wants k and v of one
    shape.  With T = 1 and g = 1 the one token sees every valid key and the result has the bits of ``sageattn_splitkv``.

    K smoothing always on, V not smoothed, ``per_warp`` or ``per_thread`` scales.  ``attn_mask``, ``block_map`` / ``plan``,
    ``cu_seqlens_q`` / ``cu_seqlens_k``, ``smooth_k=False`` and ``smooth_v`` are refused by name (ValueError), and so is
    ``is_causal=False``: the operator has no non-causal form to offer, that is ``sageattn_splitkv``."""
    kv_lens, num_splits, M = _splitkv_front("sageattn_splitkv_causal", True, q, k, v, kv_lens, num_splits, tensor_layout,
                                            pv, qk_quant_gran, refused)
    if isinstance(q_fold, bool) or not isinstance(q_fold, int):
        raise TypeError(f"q_fold must be an int >= 1, got {type(q_fold).__name__}")
    if q_fold < 1 or M % q_fold != 0:
        raise ValueError(f"q_fold must be >= 1 and divide the {M} query rows, got {q_fold}")
    return _splitkv_run(q, k, v, kv_lens, num_splits, tensor_layout, sm_scale, pv, qk_quant_gran, return_lse, q_fold=q_fold)


# ---- block-sparse attention ------------------------------------------------------------------------------------------------
class BlockSparsePlan:
    """The compacted form of a block map (``block_sparse_plan``): per (batch, query head, 128-row q-block) the ascending
    list of active 64-key tiles, as the attention kernel reads it.  A static pattern is compacted once and the plan reused
    across layers and diffusion steps."""
    __slots__ = ("lists", "B", "Hq", "M", "N")

    def __init__(self, lists, B, Hq, M, N):
        self.lists, self.B, self.Hq, self.M, self.N = lists, B, Hq, M, N


@functools.lru_cache(maxsize=64)
def _plan_ints(B, Hq, M, N):
    """int32 entries of the lists of a plan: the library's own sizing, so that the row layout is written down once"""
    return L.lib().sage_block_sparse_workspace_bytes(B, Hq, M, N) // 4


def _check_block_map(block_map, B, Hq, M, N):
    """[B|1, Hq|1, ceil(M/128), ceil(N/64)] bool / uint8 -> the [B,Hq,..] view (0 strides where it broadcasts)"""
    if not isinstance(block_map, torch.Tensor):
        raise TypeError("block_map must be a bool/uint8 tensor or a BlockSparsePlan")
    if block_map.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"block_map must be of dtype bool or uint8, got {block_map.dtype}")
    want = ((M + 127) // 128, (N + 63) // 64)
    if (block_map.dim() != 4 or tuple(block_map.shape[2:]) != want or block_map.size(0) not in (1, B)
            or block_map.size(1) not in (1, Hq)):
        raise ValueError(f"block_map shape {tuple(block_map.shape)} does not match [B={B} or 1, Hq={Hq} or 1, "
                         f"ceil(M/128)={want[0]}, ceil(N/64)={want[1]}]")
    return block_map.expand(B, Hq, *want)


def block_sparse_plan(block_map: torch.Tensor, M: int, N: int, B: Optional[int] = None, Hq: Optional[int] = None):
    """Compact ``block_map`` ([B,Hq,ceil(M/128),ceil(N/64)] bool / uint8 on the GPU; any strides, sizes 1 broadcast over B
    and Hq -- pass ``B`` / ``Hq`` to broadcast to more) into a ``BlockSparsePlan`` (sage_block_map_compact: one wave per
    list, deterministic)."""
    if isinstance(block_map, torch.Tensor) and block_map.dim() == 4:
        B = block_map.size(0) if B is None else B
        Hq = block_map.size(1) if Hq is None else Hq
    m = _check_block_map(block_map, B, Hq, M, N)
    if not m.is_cuda:
        raise ValueError("block_map must be on the GPU")
    lists = torch.empty(_plan_ints(B, Hq, M, N), dtype=torch.int32, device=m.device)
    with torch.cuda.device(m.device):
        L.check(L.lib().sage_block_map_compact(m.data_ptr(), (ctypes.c_int64 * 4)(*m.stride()), B, Hq, M, N, lists.data_ptr(),
                                           lists.numel() * 4, L.stream_ptr(m.device)), "sage_block_map_compact")
    return BlockSparsePlan(lists, B, Hq, M, N)


@torch.compiler.disable
def sageattn_block_sparse(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    block_map,
    tensor_layout: str = "HND",
    sm_scale: Optional[float] = None,
    pv: str = "fp16",
    qk_quant_gran: str = "per_thread",
    smooth_k: bool = True,
    return_lse: bool = False,
    is_causal: bool = False,
    pvthreshd=None,
    return_skipped: bool = False,
    kv_lens: Optional[torch.Tensor] = None,
):
    """SageAttention over the active 128x64 tiles of a block map (SpargeAttn's ``mask_id`` geometry): ``block_map[b,h,i,j]``
    non-zero means query rows [128 i, 128 i + 128) of head h attend keys [64 j, 64 j + 64); tiles that are off are neither
    read nor computed.  ``block_map`` is a bool/uint8 tensor [B|1, Hq|1, ceil(M/128), ceil(N/64)] or a plan from
    ``block_sparse_plan``.  Non-causal; ``pv`` ("fp16" | "fp8") is explicit.  Rows of a q-block without any active tile are
    defined: o = 0, lse = -inf.  Same pre-passes and the same kernel loop as ``sageattn_qk_int8_pv_{fp16,fp8}_cuda``.

    ``pvthreshd`` (a float > 0 or an fp32 tensor [Hq]; natural-log units of the scaled logits, the units of the LSE) turns on
    SpargeAttn's second stage: a wave (32 query rows) leaves out the softmax and the P.V product of a tile, other than the
    first of its list, whose scores all lie at least ``pvthreshd`` below the running maximum of their rows (the rule:
    include/sageattn_hip.h, sage_attn_*_blocksparse_pvskip).  Every probability left out is below e^-pvthreshd.  Values of
    a tensor that are not > 0, +inf or NaN never skip.  ``return_skipped`` appends the int32 counters
    [B, Hq, ceil(M/128), 4]: how many tiles each wave skipped.  Returns o, then lse, then the counters, each when asked for.

    ``kv_lens`` (int32 [B] on q's device, read on the device only -- no host synchronisation, the call captures into a HIP
    graph) gives every batch its own number of valid keys, ``len_b = clamp(kv_lens[b], 0, N)``: tiles at or beyond
    ``ceil(len_b / 64)`` count as off, the last valid tile is masked at ``len_b``, and the K (and FP8 V) statistics are
    taken over the valid rows only, so nothing in rows >= len_b of k or v influences any output, NaN and Inf included.  For
    len_b > 0, ``o[b]``, ``lse[b]`` and the counters of batch b are bit-identical to this operator called on ``q[b:b+1]``, the
    first len_b keys of ``k[b:b+1]`` / ``v[b:b+1]`` and the map cut to ``ceil(len_b / 64)`` columns; a q-block left without
    a tile -- every q-block of a batch without keys -- gives o = 0, lse = -inf, counters 0.  The map or plan is that of N
    and is not modified: one plan serves any lengths.  Needs ``smooth_k=True``; ``pv="fp8"`` wants k and v of one shape.
    The rule: include/sageattn_hip.h, per-batch key lengths for block-sparse attention."""
    _check_pvskip_args(pvthreshd, return_skipped)
    if is_causal:  # accepted only to be refused by name: unknown keywords are a TypeError
        raise ValueError("sageattn_block_sparse is non-causal: express the causal structure in the block map")
    _check_sparse_args(pv, qk_quant_gran, tensor_layout)
    B, Hq, M, _ = L.dims(q, tensor_layout)
    N = L.dims(k, tensor_layout)[2]
    kv_lens = _check_sparse_kv_lens(kv_lens, q, k, v, pv, smooth_k)
    if isinstance(block_map, BlockSparsePlan):
        if (block_map.B, block_map.Hq, block_map.M, block_map.N) != (B, Hq, M, N):
            raise ValueError(f"the plan was made for (B, Hq, M, N) = {(block_map.B, block_map.Hq, block_map.M, block_map.N)}, "
                             f"the call has {(B, Hq, M, N)}")
        need = _plan_ints(B, Hq, M, N)
        if block_map.lists.dtype != torch.int32 or block_map.lists.numel() != need or not block_map.lists.is_contiguous():
            raise ValueError(f"the plan's lists must be {need} contiguous int32, as block_sparse_plan makes them")
        map_dev = block_map.lists.device
    else:
        block_map = _check_block_map(block_map, B, Hq, M, N)
        map_dev = block_map.device
    if map_dev != q.device:
        raise ValueError(f"block_map is on {map_dev}, q on {q.device}")

    def plan_from(q, k, km, sm_scale):
        return block_map if isinstance(block_map, BlockSparsePlan) else block_sparse_plan(block_map, M, N)
    return _block_sparse_tail(q, k, v, tensor_layout, sm_scale, (pv, qk_quant_gran, smooth_k), plan_from,
                              (return_lse, False, pvthreshd, return_skipped), kv_lens)


def _check_sparse_kv_lens(kv_lens, q, k, v, pv, smooth_k):
    """The ``kv_lens`` keyword of the block-sparse operators, checked before any device call -> the tensor or None"""
    if kv_lens is None:
        return None
    kv_lens = _check_kv_lens(kv_lens, q.size(0), q.device)
    if not smooth_k:
        raise ValueError("kv_lens needs smooth_k=True: the length-aware K pre-pass always smooths")
    if pv == "fp8" and k.shape != v.shape:
        raise ValueError(f"pv='fp8' with kv_lens needs k and v of one shape, got {tuple(k.shape)} and {tuple(v.shape)}")
    return kv_lens


def _check_sparse_args(pv, qk_quant_gran, tensor_layout):
    if pv not in ("fp16", "fp8"):
        raise ValueError(f"pv must be 'fp16' or 'fp8', got {pv}")
    if qk_quant_gran not in ("per_warp", "per_thread"):
        raise ValueError("qk_quant_gran must be either 'per_warp' or 'per_thread'.")
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")


def _pack(o, lse, plan, skipped):
    """The return value of an operator: o, then lse, plan and skipped in this order, each unless None."""
    out = tuple(x for x in (o, lse, plan, skipped) if x is not None)
    return out if len(out) > 1 else out[0]


def _block_sparse_tail(q, k, v, tensor_layout, sm_scale, quant, plan_from, want, kv_lens=None):
    """What ``sageattn_block_sparse`` and ``sageattn_sparge`` do below their argument checks: pad, the K (or K + V)
    pre-pass, the plan -- ``plan_from(q, k, km, sm_scale)`` on the padded views and the smoothing mean --, the block-sparse
    attention kernel and the return tuple.  ``quant`` = (pv, qk_quant_gran, smooth_k), ``want`` = (return_lse, return_plan,
    pvthreshd, return_skipped).  With ``kv_lens`` the length-aware pre-pass and the ``_blocksparse_kvlen`` kernels."""
    pv, qk_quant_gran, smooth_k = quant
    return_lse, return_plan, pvthreshd, return_skipped = want
    _common_checks(q, k, v)
    with torch.cuda.device(q.device):
        q, k, v, head_dim_og = _pad_head_dim(q, k, v)
        if sm_scale is None:
            sm_scale = head_dim_og ** -0.5
        kv = _prepass(k, v, tensor_layout, qk_quant_gran, smooth_k, pv == "fp8", False, kv_lens)
        plan = plan_from(q, k, kv[2], sm_scale)
        thr, skipped = _pvskip_tensors(pvthreshd, return_skipped, plan.B, plan.Hq, plan.M, q.device)
        o, lse = _fused_attn(q, kv, tensor_layout, False, (qk_quant_gran, 32), sm_scale, return_lse, (plan, thr, skipped),
                             kv_lens=kv_lens)
        return _pack(o[..., :head_dim_og], lse, plan if return_plan else None, skipped)


# ---- block-map predictor -----------------------------------------------------------------------------------------------------
def _per_head(value, Hq, device, name):
    """A threshold as the fp32 [Hq] device tensor the selection kernel reads: a float is broadcast, a tensor checked."""
    if isinstance(value, torch.Tensor):
        if tuple(value.shape) != (Hq,):
            raise ValueError(f"{name} must be a float or a tensor of shape [Hq={Hq}], got {tuple(value.shape)}")
        return value.to(device=device, dtype=torch.float32).contiguous()
    return torch.full((Hq,), float(value), dtype=torch.float32, device=device)


def _check_pvskip_args(pvthreshd, return_skipped):
    """The keywords of the P.V skip, checked before anything touches a tensor.  A per-head tensor is not read here (no host
    synchronisation): the kernel takes values that are not > 0, +inf and NaN as "never skip"."""
    if pvthreshd is None:
        if return_skipped:
            raise ValueError("return_skipped needs pvthreshd: without it nothing is skipped and nothing counted")
    elif not isinstance(pvthreshd, torch.Tensor) and not float(pvthreshd) > 0.0:
        raise ValueError(f"pvthreshd must be > 0 (natural-log units of the scaled logits), got {pvthreshd}")


def _pvskip_tensors(pvthreshd, return_skipped, B, Hq, M, device):
    """-> (fp32 [Hq] thresholds or None, int32 [B,Hq,ceil(M/128),4] counters or None); every counter is written by the call"""
    if pvthreshd is None:
        return None, None
    thr = _per_head(pvthreshd, Hq, device, "pvthreshd")
    skipped = torch.empty((B, Hq, (M + 127) // 128, 4), dtype=torch.int32, device=device) if return_skipped else None
    return thr, skipped


def _check_select_args(topk, keep_first, keep_last):
    """The selection's keywords, checked before anything touches a tensor.  A per-head ``topk`` tensor is not read here (no
    host synchronisation): the kernel takes values <= 0 as "one candidate" and NaN as 1."""
    if topk is not None and not isinstance(topk, torch.Tensor) and not float(topk) > 0.0:
        raise ValueError(f"topk must be a fraction > 0 (1 and above keep every candidate), got {topk}")
    for name, value in (("keep_first", keep_first), ("keep_last", keep_last)):
        if isinstance(value, bool) or not isinstance(value, int) or value < 0:
            raise ValueError(f"{name} must be an int >= 0 (a number of 64-key blocks), got {value!r}")


def _sparge_predict(q, k, km, tensor_layout, sm_scale, want_map, select, kv_lens=None):
    """sage_block_pool_sim on q (128-row blocks) and on k - km (64-row blocks), then sage_block_select with ``select`` =
    (simthreshd1, cdfthreshd, topk, keep_first, keep_last): rule TOPK when ``topk`` is given, else CDF -> (plan, uint8 map or
    None).  q and k are padded ABI views, km [B,Hk,D] in their dtype.  With ``kv_lens`` (int32 [B]) the ``_kvlen`` twins: K is
    pooled over the valid rows of every batch and the rule runs over its ceil(len_b / 64) key blocks."""
    simthreshd1, cdfthreshd, topk, keep_first, keep_last = select
    B, Hq, M, D = L.dims(q, tensor_layout)
    _, Hk, N, _ = L.dims(k, tensor_layout)
    if Hq % Hk != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({Hk})")
    thr = _per_head(simthreshd1, Hq, q.device, "simthreshd1")
    if topk is None:
        rule, par = L.SELECT_CDF, _per_head(cdfthreshd, Hq, q.device, "cdfthreshd")
    else:
        rule, par = L.SELECT_TOPK, _per_head(topk, Hq, q.device, "topk")
    pq, sq = block_pool_sim(q, 128, tensor_layout)
    pk, sk = block_pool_sim(k, 64, tensor_layout, mean=km, kv_lens=kv_lens)
    lists = torch.empty(_plan_ints(B, Hq, M, N), dtype=torch.int32, device=q.device)
    bmap = torch.empty((B, Hq, (M + 127) // 128, (N + 63) // 64), dtype=torch.uint8, device=q.device) if want_map else None
    ntk = (N + 63) // 64  # keeps beyond it act as ntk
    args = (pq.data_ptr(), sq.data_ptr(), pk.data_ptr(), sk.data_ptr(), B, Hq, Hk, M, N, D, float(sm_scale), thr.data_ptr(),
            rule, par.data_ptr(), min(keep_first, ntk), min(keep_last, ntk), lists.data_ptr(), lists.numel() * 4, L.ptr(bmap))
    if kv_lens is None:
        L.check(L.lib().sage_block_select(*args, L.stream_ptr(q.device)), "sage_block_select")
    else:
        L.check(L.lib().sage_block_select_kvlen(*args, kv_lens.data_ptr(), L.stream_ptr(q.device)), "sage_block_select_kvlen")
    return BlockSparsePlan(lists, B, Hq, M, N), bmap


def sparge_plan(q: torch.Tensor, k: torch.Tensor, tensor_layout: str = "HND", simthreshd1=0.6, cdfthreshd=0.98,
                sm_scale: Optional[float] = None, km: Optional[torch.Tensor] = None, return_map: bool = False,
                topk=None, keep_first: int = 0, keep_last: int = 0, kv_lens: Optional[torch.Tensor] = None):
    """Predict the block map of ``sageattn_block_sparse`` from Q and K (the rule: include/sageattn_hip.h,
    sage_block_select): pooled 128-row q-blocks against pooled 64-row key blocks of ``k - km``, per q-block the fewest key
    blocks that hold ``cdfthreshd`` of the softmax mass, and every tile of a block whose rows are not alike (mean cosine
    similarity <= ``simthreshd1``).  Thresholds are floats or fp32 tensors [Hq]; ``km`` defaults to ``k_mean(k)``, the
    smoothing mean of the K quantizer.  Returns a ``BlockSparsePlan``, with ``return_map=True`` also the bool map
    [B,Hq,ceil(M/128),ceil(N/64)].  Non-causal.

    ``topk`` (a float > 0 or an fp32 tensor [Hq]) selects by budget instead: per q-block the ``ceil(topk * n)`` best-scoring
    of the head's n candidate key blocks, so that every self-similar q-block of a head gets a list of the same length;
    ``cdfthreshd`` is then not read.  ``keep_first`` / ``keep_last`` (ints >= 0) pin the first / last key blocks on under
    either rule (text tokens, an attention sink): they are always computed and take no part in the selection.

    ``kv_lens`` (int32 [B] on q's device, read on the device only): batch b has the key blocks below ``ceil(len_b / 64)``,
    ``len_b = clamp(kv_lens[b], 0, N)`` -- the last of them pooled over its valid rows, ``keep_last`` pinning the last valid
    blocks, n and the budget counted among them -- and its list rows equal those of this function on ``q[b:b+1]`` and the
    first len_b keys of ``k[b:b+1]``; map columns beyond are False, and a batch without keys gets empty lists.  ``km``
    then defaults to the length-aware smoothing mean, the one the attention call will smooth with.  That default is heavy for
    a planning call: it runs the whole length-aware K pre-pass (``k_smooth_quant_kvlen``: an INT8 K tensor, its scales and a
    workspace are allocated and written) and keeps only the mean -- pass ``km`` when the mean is at hand
    (``sageattn_sparge`` does: its pre-pass runs once).  The plan is for (B, Hq, M, N)."""
    _check_select_args(topk, keep_first, keep_last)
    if kv_lens is not None:
        kv_lens = _check_kv_lens(kv_lens, q.size(0), q.device)
    assert q.is_cuda, "Input tensors must be on cuda."
    assert q.dtype in [torch.float16, torch.bfloat16], "Input tensors must be in dtype of torch.float16 or torch.bfloat16"
    assert q.device == k.device and q.dtype == k.dtype, "q and k must have one device and one dtype."
    with torch.cuda.device(q.device):
        q, k, _, head_dim_og = _pad_head_dim(q, k, k)
        if sm_scale is None:
            sm_scale = head_dim_og ** -0.5
        if km is None and kv_lens is not None:  # the mean over the valid rows: what the length-aware K pre-pass smooths with
            km = k_smooth_quant_kvlen(k, kv_lens, tensor_layout, L.GRAN_PER_THREAD, L.ROUND_TRITON)[2]
        elif km is None:
            km = k_mean(k, tensor_layout)
        else:
            km = torch.nn.functional.pad(km, (0, k.size(-1) - km.size(-1))).to(k.dtype).contiguous()
        plan, bmap = _sparge_predict(q, k, km, tensor_layout, sm_scale, return_map,
                                     (simthreshd1, cdfthreshd, topk, keep_first, keep_last), kv_lens)
    return (plan, bmap.view(torch.bool)) if return_map else plan


@torch.compiler.disable
def sageattn_sparge(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    tensor_layout: str = "HND",
    simthreshd1=0.6,
    cdfthreshd=0.98,
    sm_scale: Optional[float] = None,
    pv: str = "fp16",
    qk_quant_gran: str = "per_thread",
    return_lse: bool = False,
    return_plan: bool = False,
    topk=None,
    keep_first: int = 0,
    keep_last: int = 0,
    pvthreshd=None,
    return_skipped: bool = False,
    kv_lens: Optional[torch.Tensor] = None,
):
    """``sageattn_block_sparse`` on the block map that ``sparge_plan`` predicts for this q and k: the K (or K + V) pre-pass
    runs once, the predictor uses its smoothing mean, and the block-sparse attention kernel reads the predicted lists.
    Bit-identical to ``sageattn_block_sparse(q, k, v, sparge_plan(q, k, ...))``.  Returns o, then the LSE with
    ``return_lse``, then the ``BlockSparsePlan`` with ``return_plan``.  Non-causal.  ``topk``, ``keep_first`` and
    ``keep_last`` as for ``sparge_plan``: with ``topk`` the budget rule is used and ``cdfthreshd`` is not read.
    ``pvthreshd`` and ``return_skipped`` as for ``sageattn_block_sparse`` (SpargeAttn's second stage, on the predicted
    tiles); the counters come last: o, lse, plan, skipped.  ``kv_lens`` (int32 [B] on q's device) as for ``sparge_plan`` and
    ``sageattn_block_sparse``: bit-identical to ``sageattn_block_sparse(q, k, v, sparge_plan(q, k, ..., kv_lens=kv_lens),
    kv_lens=kv_lens)``."""
    _check_select_args(topk, keep_first, keep_last)
    _check_pvskip_args(pvthreshd, return_skipped)
    _check_sparse_args(pv, qk_quant_gran, tensor_layout)
    kv_lens = _check_sparse_kv_lens(kv_lens, q, k, v, pv, True)

    select = (simthreshd1, cdfthreshd, topk, keep_first, keep_last)

    def plan_from(q, k, km, sm_scale):
        return _sparge_predict(q, k, km, tensor_layout, sm_scale, False, select, kv_lens)[0]
    return _block_sparse_tail(q, k, v, tensor_layout, sm_scale, (pv, qk_quant_gran, True), plan_from,
                              (return_lse, return_plan, pvthreshd, return_skipped), kv_lens)


# ---- calibration of the predictor ------------------------------------------------------------------------------------------------
def _tile_mass(q, k8, ks, km, tensor_layout, qk_quant_gran, sm_scale, kv_lens=None):
    """sage_attn_tile_mass on the padded query view ``q`` and the K operands of ``_prep_k`` -> fp32 [B,Hq,nqb,ntk].  With
    ``kv_lens`` (int32 [B]) sage_attn_tile_mass_kvlen on the K operands of ``k_smooth_quant_kvlen``."""
    B, Hq, M, D = L.dims(q, tensor_layout)
    _, Hk, N, _ = L.dims(k8, tensor_layout)
    if Hq % Hk != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({Hk})")
    q8, qs, _ = _quant_q(q, km, tensor_layout, qk_quant_gran, sm_scale, 32, False, Hq, Hk)
    mass = torch.empty((B, Hq, (M + 127) // 128, (N + 63) // 64), dtype=torch.float32, device=q.device)
    args = (L.desc(q8, tensor_layout), L.desc(k8, tensor_layout), qs.data_ptr(), ks.data_ptr(), B, Hq, Hk, M, N, D,
            _GRAN_CODE[qk_quant_gran], 128, 32, float(sm_scale), 0, mass.data_ptr())
    if kv_lens is None:
        L.check(L.lib().sage_attn_tile_mass(*args, L.stream_ptr(q.device)), "sage_attn_tile_mass")
    else:
        L.check(L.lib().sage_attn_tile_mass_kvlen(*args, kv_lens.data_ptr(), L.stream_ptr(q.device)),
                "sage_attn_tile_mass_kvlen")
    return mass


def _check_kv_lens_kind(kv_lens):
    """What ``_check_kv_lens`` asks of ``kv_lens`` alone -- an int32 tensor of one dimension --, for the functions that check
    it before they look at any other argument; [B] and the device follow in ``_check_kv_lens``"""
    if not isinstance(kv_lens, torch.Tensor):
        raise TypeError("kv_lens must be an int32 tensor of shape [B]")
    if kv_lens.dtype != torch.int32:
        raise TypeError(f"kv_lens must be of dtype int32, got {kv_lens.dtype}")
    if kv_lens.dim() != 1:
        raise ValueError(f"kv_lens shape {tuple(kv_lens.shape)} does not match [B]")


def sageattn_tile_mass(q: torch.Tensor, k: torch.Tensor, tensor_layout: str = "HND", sm_scale: Optional[float] = None,
                       qk_quant_gran: str = "per_thread", smooth_k: bool = True):
    """The exact softmax mass of every 128x64 tile of ``sageattn_block_sparse(q, k, ...)`` with the same ``qk_quant_gran`` and
    ``smooth_k``: fp32 [B,Hq,ceil(M/128),ceil(N/64)], per q-block the probabilities of the dense operator summed over the
    tile's keys and averaged over the block's valid rows (the definition: include/sageattn_hip.h, sage_attn_tile_mass).  It
    is computed from the INT8 Q and K and the scales that operator multiplies -- same head-dim padding, K pre-pass and Q
    quantizer -- so each row of the last axis sums to 1 and ``plan_recall`` of a map is the share of the probability that the
    map keeps.  Costs about one dense attention call.  Non-causal.  There is no ``kv_lens`` keyword here (a TypeError, as
    every unknown keyword) and the mass of a padded batch includes its padding: per-batch key lengths are the twin
    ``sageattn_tile_mass_kvlen``."""
    _check_sparse_args("fp16", qk_quant_gran, tensor_layout)
    return _tile_mass_of(q, k, None, tensor_layout, sm_scale, qk_quant_gran, smooth_k)


def _tile_mass_of(q, k, kv_lens, tensor_layout, sm_scale, qk_quant_gran, smooth_k):
    """``sageattn_tile_mass`` and its twin below their argument checks"""
    assert q.is_cuda, "Input tensors must be on cuda."
    assert q.dtype in [torch.float16, torch.bfloat16], "Input tensors must be in dtype of torch.float16 or torch.bfloat16"
    assert q.device == k.device and q.dtype == k.dtype, "q and k must have one device and one dtype."
    with torch.cuda.device(q.device):
        q, k, _, head_dim_og = _pad_head_dim(q, k, k)
        if sm_scale is None:
            sm_scale = head_dim_og ** -0.5
        if kv_lens is None:
            k8, ks, km = _prep_k(k, tensor_layout, qk_quant_gran, smooth_k)
        else:
            k8, ks, km = k_smooth_quant_kvlen(k, kv_lens, tensor_layout, *_k_pairing(qk_quant_gran))
        return _tile_mass(q, k8, ks, km, tensor_layout, qk_quant_gran, sm_scale, kv_lens)


def sageattn_tile_mass_kvlen(q: torch.Tensor, k: torch.Tensor, kv_lens: torch.Tensor, tensor_layout: str = "HND",
                             sm_scale: Optional[float] = None, qk_quant_gran: str = "per_thread"):
    """``sageattn_tile_mass`` with a per-batch number of valid keys: the exact tile mass of what
    ``sageattn_block_sparse(q, k, ..., kv_lens=kv_lens)`` multiplies.  ``kv_lens`` is an int32 [B] tensor on q's device, read
    on the device only (no host synchronisation; the call captures into a HIP graph and a replay reads the lengths the tensor
    holds then); ``len_b = clamp(kv_lens[b], 0, N)``, ``ntk_b = ceil(len_b / 64)``.

    For every b with len_b > 0, ``mass[b, :, :, :ntk_b]`` is bit-identical to ``sageattn_tile_mass`` on ``q[b:b+1]`` and the
    first len_b keys of ``k[b:b+1]`` with the same ``qk_quant_gran``; the entries ``[ntk_b, ceil(N/64))`` are exactly 0, and
    every entry is written by every call.  A batch without keys has an all-zero row -- the one exception to "every
    ``mass[b,h,i,:]`` sums to 1".  Nothing in rows >= len_b of k influences anything, NaN and Inf included: the smoothing mean
    and the K scales are those of the length-aware K pre-pass (``k_smooth_quant_kvlen``), taken over the valid rows, and the
    kernel neither loads rows nor scales beyond them.  K smoothing is always on (that pre-pass always smooths): there is no
    ``smooth_k``.  The rule: include/sageattn_hip.h, sage_attn_tile_mass_kvlen."""
    _check_kv_lens_kind(kv_lens)
    _check_sparse_args("fp16", qk_quant_gran, tensor_layout)
    kv_lens = _check_kv_lens(kv_lens, q.size(0), q.device)
    return _tile_mass_of(q, k, kv_lens, tensor_layout, sm_scale, qk_quant_gran, True)


def _plan_recall(plan, mass, kv_lens=None):
    recall = torch.empty(mass.shape[:3], dtype=torch.float32, device=mass.device)
    kept = torch.empty(mass.shape[:3], dtype=torch.int32, device=mass.device)
    args = (plan.lists.data_ptr(), plan.lists.numel() * 4, mass.data_ptr(), plan.B, plan.Hq, plan.M, plan.N, recall.data_ptr(),
            kept.data_ptr())
    if kv_lens is None:
        L.check(L.lib().sage_block_plan_recall(*args, L.stream_ptr(mass.device)), "sage_block_plan_recall")
    else:
        L.check(L.lib().sage_block_plan_recall_kvlen(*args, kv_lens.data_ptr(), L.stream_ptr(mass.device)),
                "sage_block_plan_recall_kvlen")
    return recall, kept


def plan_recall(plan_or_map, mass: torch.Tensor):
    """What a plan keeps of ``mass`` (``sageattn_tile_mass``): (recall fp32 [B,Hq,nqb], kept int32 [B,Hq,nqb]) -- per q-block
    the summed mass of its active tiles and their number (sage_block_plan_recall: deterministic, and never smaller for a
    superset of tiles).  ``plan_or_map`` is a ``BlockSparsePlan`` or a bool / uint8 map [B|1, Hq|1, nqb, ntk], which is
    compacted with ``block_sparse_plan`` first.  An empty q-block has recall 0.  No ``kv_lens`` keyword: every listed tile
    counts (in a plan made with lengths the tiles beyond a batch's length are off already); ``plan_recall_kvlen`` clips any
    plan or map to per-batch key lengths."""
    return _plan_recall_of(plan_or_map, mass, None)


def plan_recall_kvlen(plan_or_map, mass: torch.Tensor, kv_lens: torch.Tensor):
    """``plan_recall`` under per-batch key lengths (``kv_lens`` int32 [B] on the device of ``mass``, read on the device only;
    ``ntk_b = ceil(clamp(kv_lens[b], 0, N) / 64)`` with N = 64 ntk for a map, the plan's N for a plan):
    ``recall[b,h,i]`` is the sum of ``mass[b,h,i,j]`` over the listed tiles j < ntk_b and ``kept[b,h,i]`` the number of those
    entries -- what ``sageattn_block_sparse(..., kv_lens=kv_lens)`` computes of the list.  The sum runs in the tile slots and
    the fixed tree of ``plan_recall``, so it is bit-identical to ``plan_recall`` on the map and the mass both cut to ntk_b
    columns, and as monotone under set inclusion.  The clip is by list entry: it does not rely on ``mass`` being 0 beyond the
    length (``sageattn_tile_mass_kvlen`` writes 0 there all the same).  The lists are only read: a plan made without
    lengths, or a static map, serves any lengths.  A batch without keys has recall 0 and kept 0."""
    _check_kv_lens_kind(kv_lens)
    return _plan_recall_of(plan_or_map, mass, kv_lens)


def _plan_recall_of(plan_or_map, mass, kv_lens):
    """``plan_recall`` and its twin: the checks of mass and plan, the compaction of a map, the launch"""
    if not isinstance(mass, torch.Tensor) or mass.dim() != 4 or mass.dtype != torch.float32:
        raise ValueError("mass must be the fp32 [B,Hq,ceil(M/128),ceil(N/64)] tensor of sageattn_tile_mass")
    B, Hq, nqb, ntk = mass.shape
    if kv_lens is not None:
        kv_lens = _check_kv_lens(kv_lens, B, mass.device)
    if isinstance(plan_or_map, BlockSparsePlan):
        plan = plan_or_map
        if (plan.B, plan.Hq, (plan.M + 127) // 128, (plan.N + 63) // 64) != (B, Hq, nqb, ntk):
            raise ValueError(f"the plan was made for (B, Hq, M, N) = {(plan.B, plan.Hq, plan.M, plan.N)}, mass has the shape "
                             f"{tuple(mass.shape)}")
        if plan.lists.dtype != torch.int32 or plan.lists.numel() != _plan_ints(plan.B, plan.Hq, plan.M, plan.N):
            raise ValueError("the plan's lists must be as block_sparse_plan makes them")
    else:
        if not isinstance(plan_or_map, torch.Tensor):
            raise TypeError("plan_or_map must be a BlockSparsePlan or a bool/uint8 block map")
        if plan_or_map.dim() != 4 or tuple(plan_or_map.shape[2:]) != (nqb, ntk):
            raise ValueError(f"block map shape {tuple(plan_or_map.shape)} does not match the mass {tuple(mass.shape)}")
        plan = block_sparse_plan(plan_or_map, nqb * 128, ntk * 64, B, Hq)  # whole blocks: the lists depend on the counts only
    if plan.lists.device != mass.device:
        raise ValueError(f"the plan is on {plan.lists.device}, mass on {mass.device}")
    with torch.cuda.device(mass.device):
        return _plan_recall(plan, mass.contiguous(), kv_lens)


class SpargeTuning:
    """The result of ``sparge_tune``; every tensor has shape [Hq] and lives on the device.
    ``rule`` "cdf" | "topk";  ``param`` fp32, the tuned ``cdfthreshd`` / ``topk`` -- pass it to ``sageattn_sparge`` as it is;
    ``met`` bool, False where even 1.0 misses the target (``param`` is then 1.0);  ``recall`` the head recall at ``param``;
    ``recall_below`` that at ``param - 2^-steps`` (-inf where that is 0);  ``density`` kept tiles over all tiles at ``param``."""
    __slots__ = ("rule", "param", "met", "recall", "recall_below", "density")

    def __init__(self, rule, param, met, recall, recall_below, density):
        self.rule, self.param, self.met = rule, param, met
        self.recall, self.recall_below, self.density = recall, recall_below, density

    def __repr__(self):
        return (f"SpargeTuning(rule={self.rule!r}, param={self.param}, met={self.met}, recall={self.recall}, "
                f"recall_below={self.recall_below}, density={self.density})")


def sparge_tune(q: torch.Tensor, k: torch.Tensor, tensor_layout: str = "HND", target: float = 0.95, rule: str = "cdf",
                simthreshd1=0.6, keep_first: int = 0, keep_last: int = 0, steps: int = 8, reduce: str = "mean",
                sm_scale: Optional[float] = None, qk_quant_gran: str = "per_thread", mass: Optional[torch.Tensor] = None):
    """Tune the predictor on data: per query head the smallest ``cdfthreshd`` (``rule="cdf"``) or ``topk`` (``rule="topk"``)
    on the grid g / 2^steps, g = 1 .. 2^steps, at which the predicted map keeps at least ``target`` of the exact softmax mass
    (``sageattn_tile_mass``; pass ``mass`` to reuse one).  The head recall is, with ``reduce="mean"``, the mean over batches
    and q-blocks of ``plan_recall`` weighted by the blocks' valid rows -- the mean captured probability per query row --
    and with ``"min"`` the minimum.  ``simthreshd1``, ``keep_first`` and ``keep_last`` are fixed inputs, as for
    ``sparge_plan``.  Returns a ``SpargeTuning``.

    Cost: Q and K are pooled once, the mass is computed once, and the search is one selection at 1.0 and then ``steps``
    bisection steps, each one sage_block_select with the per-head candidates, one sage_block_plan_recall and a few
    reductions on [Hq] tensors -- never a run of sparse attention.  Nothing is read back to the host: no synchronisation, and
    the function captures into a HIP graph.

    Why bisection finds the smallest grid value exactly: under both rules the tiles a q-block keeps at a larger parameter
    are a superset of those at a smaller one -- either rule takes a prefix of one ranking of the candidates, and the tiles of
    blocks that are not self-similar or are pinned on do not depend on the parameter.  sage_block_plan_recall adds the
    non-negative mass in fixed tile slots and a fixed tree, so a superset never sums to less, and the reductions over batches
    and q-blocks are fixed-order sums or minima of these.  Head recall is therefore monotone in the parameter, in fp32 as
    well as in exact arithmetic, and the grid splits into a failing part below ``param`` and a passing part from it on.

    There is no ``kv_lens`` keyword here (a TypeError) and a padded batch is tuned with its padding: per-batch key lengths
    are the twin ``sparge_tune_kvlen``."""
    _check_tune_args(target, rule, keep_first, keep_last, steps, reduce, qk_quant_gran, tensor_layout)
    return _sparge_tune(q, k, None, tensor_layout, target, rule, simthreshd1, keep_first, keep_last, steps, reduce, sm_scale,
                        qk_quant_gran, mass)


def sparge_tune_kvlen(q: torch.Tensor, k: torch.Tensor, kv_lens: torch.Tensor, tensor_layout: str = "HND",
                      target: float = 0.95, rule: str = "cdf", simthreshd1=0.6, keep_first: int = 0, keep_last: int = 0,
                      steps: int = 8, reduce: str = "mean", sm_scale: Optional[float] = None,
                      qk_quant_gran: str = "per_thread", mass: Optional[torch.Tensor] = None):
    """``sparge_tune`` for a padded batch with per-batch key lengths: the parameter that
    ``sageattn_sparge(q, k, v, ..., kv_lens=kv_lens)`` needs to keep ``target`` of the mass of the keys it attends.
    ``kv_lens`` is an int32 [B] tensor on q's device, read on the device only (no host synchronisation; the function captures
    into a HIP graph and a replay reads the lengths the tensor holds then); ``len_b = clamp(kv_lens[b], 0, N)``,
    ``ntk_b = ceil(len_b / 64)``.  Returns a ``SpargeTuning``.

    It is the search of ``sparge_tune`` with four substitutions: the smoothing mean (and, for the mass, the INT8 K and its
    scales) come from the length-aware K pre-pass ``k_smooth_quant_kvlen``; K is pooled with
    ``block_pool_sim(..., kv_lens=kv_lens)``; the selection is sage_block_select_kvlen, what ``sparge_plan(...,
    kv_lens=kv_lens)`` runs; and the recall is ``plan_recall_kvlen`` of ``sageattn_tile_mass_kvlen`` (pass ``mass`` to reuse
    one).  When ``mass`` is passed the K pre-pass still runs, whole, to get that mean -- the heavy default ``sparge_plan``
    describes for its ``km``.

    Batches without keys take no part in the reductions.  With ``rec, kept = plan_recall_kvlen(plan, mass, kv_lens)``,
    ``weight`` the valid rows of the q-blocks as fp32 [1,1,nqb], ``lens = kv_lens.clamp(0, N)``, ``valid = lens > 0``,
    ``nv = valid.sum()`` and ``ntk_b = (lens + 63) // 64``, all on the device and in fp32:
      ``"mean"``   ``(rec * weight * valid[:, None, None]).sum((0, 2)) * (nv.clamp(min=1) * M).to(torch.float32).reciprocal()``
      ``"min"``    ``torch.where(valid[:, None, None], rec, inf).amin((0, 2))``
      density      ``kept.sum((0, 2)).to(torch.float32) * (nqb * ntk_b.sum()).clamp(min=1).to(torch.float32).reciprocal()``
    (the product with a reciprocal, not a quotient, because that is what torch makes of ``sparge_tune``'s division by the
    Python number ``B * M``: with all lengths equal to N every field of the result is bit-identical to ``sparge_tune(q, k,
    ...)``).  When no batch has keys (``nv == 0``) the head recall is 1 and the density 0, so ``param`` is ``2^-steps`` and
    ``met`` True.

    The monotonicity argument of ``sparge_tune`` carries over unchanged: sage_block_select_kvlen keeps supersets at larger
    parameters within the ntk_b key blocks of every batch, the clipped recall adds non-negative mass in fixed tile slots and
    a fixed tree, and the reductions above are fixed-order sums or minima of it scaled by factors that do not depend on the
    parameter.  So bisection again returns the smallest passing grid value exactly."""
    _check_kv_lens_kind(kv_lens)
    _check_tune_args(target, rule, keep_first, keep_last, steps, reduce, qk_quant_gran, tensor_layout)
    kv_lens = _check_kv_lens(kv_lens, q.size(0), q.device)
    return _sparge_tune(q, k, kv_lens, tensor_layout, target, rule, simthreshd1, keep_first, keep_last, steps, reduce, sm_scale,
                        qk_quant_gran, mass)


def _check_tune_args(target, rule, keep_first, keep_last, steps, reduce, qk_quant_gran, tensor_layout):
    """The keywords of ``sparge_tune`` and its twin, checked before anything touches a tensor"""
    if rule not in ("cdf", "topk"):
        raise ValueError(f"rule must be 'cdf' or 'topk', got {rule!r}")
    if reduce not in ("mean", "min"):
        raise ValueError(f"reduce must be 'mean' or 'min', got {reduce!r}")
    if isinstance(target, bool) or not (0.0 < float(target) <= 1.0):
        raise ValueError(f"target must lie in (0, 1], got {target!r}")
    if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps <= 16:
        raise ValueError(f"steps must be an int in 1..16, got {steps!r}")
    _check_select_args(None, keep_first, keep_last)
    _check_sparse_args("fp16", qk_quant_gran, tensor_layout)


def _sparge_tune(q, k, kv_lens, tensor_layout, target, rule, simthreshd1, keep_first, keep_last, steps, reduce, sm_scale,
                 qk_quant_gran, mass):
    """The search of ``sparge_tune`` (``kv_lens`` None) and of ``sparge_tune_kvlen`` below their argument checks"""
    assert q.is_cuda, "Input tensors must be on cuda."
    assert q.dtype in [torch.float16, torch.bfloat16], "Input tensors must be in dtype of torch.float16 or torch.bfloat16"
    assert q.device == k.device and q.dtype == k.dtype, "q and k must have one device and one dtype."
    dev = q.device
    with torch.cuda.device(dev):
        q, k, _, head_dim_og = _pad_head_dim(q, k, k)
        if sm_scale is None:
            sm_scale = head_dim_og ** -0.5
        B, Hq, M, D = L.dims(q, tensor_layout)
        _, Hk, N, _ = L.dims(k, tensor_layout)
        if Hq % Hk != 0:
            raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({Hk})")
        nqb, ntk = (M + 127) // 128, (N + 63) // 64
        if mass is not None:
            if tuple(mass.shape) != (B, Hq, nqb, ntk) or mass.dtype != torch.float32 or mass.device != dev:
                raise ValueError(f"mass must be an fp32 tensor of shape {(B, Hq, nqb, ntk)} on {dev}")
            mass = mass.contiguous()
        if kv_lens is not None:  # the length-aware pre-pass: its mean is what the attention call will smooth with
            k8, ks, km = k_smooth_quant_kvlen(k, kv_lens, tensor_layout, *_k_pairing(qk_quant_gran))
            if mass is None:
                mass = _tile_mass(q, k8, ks, km, tensor_layout, qk_quant_gran, sm_scale, kv_lens)
        elif mass is None:
            k8, ks, km = _prep_k(k, tensor_layout, qk_quant_gran, True)
            mass = _tile_mass(q, k8, ks, km, tensor_layout, qk_quant_gran, sm_scale)
        else:
            km = k_mean(k, tensor_layout)
        thr = _per_head(simthreshd1, Hq, dev, "simthreshd1")
        pq, sq = block_pool_sim(q, 128, tensor_layout)
        pk, sk = block_pool_sim(k, 64, tensor_layout, mean=km, kv_lens=kv_lens)
        plan = BlockSparsePlan(torch.empty(_plan_ints(B, Hq, M, N), dtype=torch.int32, device=dev), B, Hq, M, N)
        code = L.SELECT_CDF if rule == "cdf" else L.SELECT_TOPK
        weight = (torch.arange(nqb, device=dev) * -128 + M).clamp(max=128).to(torch.float32).view(1, 1, nqb)  # c_i
        unit = 2.0 ** -steps
        if kv_lens is not None:  # the reductions the docstring of sparge_tune_kvlen states; nothing is read back
            lens = kv_lens.clamp(0, N)
            valid = (lens > 0).view(B, 1, 1)
            some = valid.any()
            weight_valid = weight * valid  # (rec * weight) * valid == rec * (weight * valid) bit for bit: valid is 0 or 1
            inv_rows = (valid.sum().clamp(min=1) * M).to(torch.float32).reciprocal()
            inv_tiles = (nqb * ((lens + 63) // 64).sum()).clamp(min=1).to(torch.float32).reciprocal()

        def evaluate(par):
            """-> (head recall, density) [Hq] of the selection with the per-head parameters ``par``"""
            args = (pq.data_ptr(), sq.data_ptr(), pk.data_ptr(), sk.data_ptr(), B, Hq, Hk, M, N, D, float(sm_scale),
                    thr.data_ptr(), code, par.data_ptr(), min(keep_first, ntk), min(keep_last, ntk), plan.lists.data_ptr(),
                    plan.lists.numel() * 4, None)
            if kv_lens is None:
                L.check(L.lib().sage_block_select(*args, L.stream_ptr(dev)), "sage_block_select")
                rec, kept = _plan_recall(plan, mass)
                if reduce == "mean":
                    head = (rec * weight).sum(dim=(0, 2)) / float(B * M)
                else:
                    head = rec.amin(dim=(0, 2))
                return head, kept.sum(dim=(0, 2)).to(torch.float32) / float(B * nqb * ntk)
            L.check(L.lib().sage_block_select_kvlen(*args, kv_lens.data_ptr(), L.stream_ptr(dev)), "sage_block_select_kvlen")
            rec, kept = _plan_recall(plan, mass, kv_lens)
            if reduce == "mean":
                head = (rec * weight_valid).sum(dim=(0, 2)) * inv_rows
            else:
                head = torch.where(valid, rec, float("inf")).amin(dim=(0, 2))
            return torch.where(some, head, 1.0), kept.sum(dim=(0, 2)).to(torch.float32) * inv_tiles

        hi = torch.full((Hq,), 1 << steps, dtype=torch.int32, device=dev)  # passes (or nothing does)
        lo = torch.zeros_like(hi)                                          # fails: the empty parameter is never evaluated
        r_hi, d_hi = evaluate(hi.to(torch.float32) * unit)
        met = r_hi >= target
        r_lo = torch.full_like(r_hi, float("-inf"))
        for _ in range(steps):
            mid = (lo + hi) // 2
            r, d = evaluate(mid.to(torch.float32) * unit)
            ok = r >= target
            hi, r_hi, d_hi = torch.where(ok, mid, hi), torch.where(ok, r, r_hi), torch.where(ok, d, d_hi)
            lo, r_lo = torch.where(ok, lo, mid), torch.where(ok, r_lo, r)
        return SpargeTuning(rule, hi.to(torch.float32) * unit, met, r_hi, r_lo, d_hi)
