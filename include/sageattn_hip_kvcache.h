/*
 * sageattn_hip_kvcache.h -- extension of the C ABI (sageattn_hip.h): a persistent quantized KV cache for the split-KV
 * attention entry points.  Same conventions: device pointers, element strides, the caller owns every buffer, every argument
 * is checked before the launch and a call that returns an argument status has enqueued nothing.
 *
 * sage_attn_fusedq_pv_{f16,f8}_splitkv[_causal] take prepared operands -- the INT8 keys k8 with their scales, the smoothing
 * vector km, and for FP8 P.V the V^T image with its per-channel scale.  A decode loop that derives them again on every call
 * quantizes keys that were quantized a step ago.  This header states the rule under which prepared operands stay valid
 * while the cache grows, and declares the one entry point that extends them in place.
 *
 * THE RULE
 *
 * Frozen smoothing vector.  Softmax is invariant to subtracting one vector from every key: q.(k - c) differs from q.k by a
 * constant per query row, and the attention kernels add (q.km) * sm_scale back into the LSE.  km therefore need not be the
 * mean of the current keys; it must only be the SAME vector for every key of a (batch, KV head).  A cache freezes
 * km[b,h,:] when it is prepared (sage_k_smooth_quant_kvlen / sage_kv_prepare_fp8_kvlen store it) and never moves it.  How
 * close it stays to the true mean decides quantization quality only; o and lse do not depend on it in real arithmetic.
 *
 * K tiles.  The scale groups of K (one per 64-key tile, or the 4 per-thread groups of it) live inside one tile, so growth
 * is local.  With start_b = clamp(start_lens[b], 0, N) and len_b = clamp(kv_lens[b], 0, N):
 *  - len_b == 0: nothing of batch b is touched.
 *  - len_b > 0: the touched tiles are t0_b .. ceil(len_b / 64) - 1, t0_b = floor(min(start_b, len_b - 1) / 64).
 *  - The INT8 rows < len_b of every touched tile, and all its scales, are bit-identical to
 *    sage_quant_qk_int8(k[b, :, :len_b], mean = km[b], is_key = 1, blk 64, warp 64, the same gran and rounding).
 *  - Rows >= len_b of k are never loaded (NaN there changes nothing); no byte of another tile and no other scale is written.
 *  - start_b >= len_b adds no rows (or follows a rollback of rejected speculative tokens): exactly the tile that holds row
 *    len_b - 1 is quantized again, ragged at len_b.
 * By induction, after any sequence of appends the valid part of the cache equals a from-scratch quantization of the current
 * prefix against the frozen km.
 *
 * FP8 V.  The per-channel scale is a statistic of the whole sequence, so it is frozen too, with headroom: the caller keeps
 * v_scale_c = headroom * v_scale (v_scale of the length-aware pre-pass, headroom >= 1) as the attention operand and hands
 * this entry point the coefficients v_coef, fp32 [B,H,2,D] as sage_quant_v_fp8_apply takes them: row 0 zeros (no V
 * smoothing), row 1 coef = 1 / v_scale_c, and 0 where v_scale_c == 0.  Later values beyond the frozen range saturate to
 * +-448: the append clamps v * coef to [-448, 448] before the conversion (the gfx950 conversion itself does not saturate,
 * beyond the range it returns the NaN byte; sage_quant_v_fp8_apply does not clamp).  Every touched 64-token block of the V^T
 * image is bit-identical to sage_quant_v_fp8_apply(v[b, :, :len_b], v_coef) in every byte that is no NaN there, its zero
 * bytes in the columns [len_b, 64 * ceil(len_b / 64)) included; where that call overflows to NaN the block holds +-448.
 * At head_dim 64 a workgroup writes two blocks and may rewrite the whole block below t0_b: the same bytes from unchanged
 * rows.  FP16 / BF16 P.V needs no V state: the caller's V buffer is the operand.
 *
 * Preconditions, stated and not checked (checking them would need a host read):
 *  - the rows < start_b of k and v are unchanged since they were quantized;
 *  - len_b - min(start_b, len_b) <= max_new, a host integer that sizes the grid: tiles beyond ceil(max_new / 64) + 1 slots
 *    from t0_b are not processed.
 *
 * Lengths are read on the device only: no host synchronisation; the call captures into a HIP graph together with the
 * attention call, and a replay reads the lengths the tensors hold then.
 *
 * NOT BUILT: dropping the caller's fp16 K buffer (the ragged tile is quantized again from its fp16 rows; without them the
 * cache would need a 64-row fp16 tail per head and a sequential walk); moving the frozen km or V scale without preparing
 * again; V smoothing and K without smoothing.  Paged / block-table caches are sageattn_hip_paged.h: this rule in logical
 * tiles, on pages of one pool.
 */
#ifndef SAGEATTN_HIP_KVCACHE_H
#define SAGEATTN_HIP_KVCACHE_H

#include "sageattn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Extend the prepared operands of a [B,H,N,D] cache by the rule above, in ONE launch of (K tile slots + V unit slots, H, B)
 * workgroups; the workgroups of slots a batch does not need return at once.
 *   k, v           the caller's fp16 / bf16 buffers (dtype); v may be NULL when v_fp8 is
 *   km             [B,H,D] in k's dtype, 16-byte aligned: the frozen smoothing vector (read only)
 *   k_int8         INT8 [B,H,N,D];  k_scale fp32 [B,H,G] contiguous, G = ceil(N/64) * (gran == per_thread ? 4 : 1)
 *   gran           SAGE_GRAN_PER_BLOCK | SAGE_GRAN_PER_THREAD;  rounding: sage_rounding
 *   v_fp8          the V^T image [B,H,D,64*ceil(N/64)] (stride_n = stride of d; 64-token blocks 64 bytes apart), or NULL: no V half
 *   v_coef         fp32 [B,H,2,D], 16-byte aligned; required with v_fp8
 *   start_lens,    int32 [B], 4-byte aligned
 *   kv_lens
 *   max_new        >= 1: the most rows any batch gains in this call
 * Checked before the launch: a NULL or misaligned pointer, B, H or N < 1, max_new < 1, v_fp8 without v or v_coef, a gran
 * other than the two (per_warp is not a K granularity here, as for sage_k_smooth_quant), an unknown rounding or dtype ->
 * SAGE_ERR_INVALID_ARGUMENT; D not 64 or 128 -> SAGE_ERR_UNSUPPORTED_HEAD_DIM. */
int sage_kv_cache_append(const sage_tensor* k, const sage_tensor* v, int dtype, int B, int H, int N, int D, const void* km,
                         const sage_tensor* k_int8, float* k_scale, int gran, int rounding, const sage_tensor* v_fp8,
                         const float* v_coef, const int32_t* start_lens, const int32_t* kv_lens, int max_new,
                         sage_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGEATTN_HIP_KVCACHE_H */
