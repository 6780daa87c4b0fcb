/*
 * sageattn_hip_decode_window.h -- extension of the C ABI (sageattn_hip_decode.h, sageattn_hip_window.h): DECODE attention with a
 * SLIDING WINDOW and SINK LOGITS on the paged cache, one wave per split, and with one split ONE launch.  gpt-oss has a sink
 * logit in every layer and a 128-key window in every other one; Mistral and Gemma 2/3 attend a window only.  Their decode steps
 * have at most 32 folded rows, for which sage_attn_fusedq_pv_*_splitkv_paged_window runs four waves where one has rows to
 * store, and a 128-key window is two or three tiles: num_splits is 1 and the merge launch only adds q . km, applies the sink
 * and rounds.  The two entry points here run the one-wave kernel of sageattn_hip_decode.h with a two-sided limit and, with
 * num_splits == 1, finish the rows in its epilogue: no second launch and no workspace.  Nothing dispatches to them implicitly.
 * Same conventions: device pointers, every argument is checked before any launch and a call that returns an argument status has
 * enqueued nothing.
 *
 * THE RULE (that of sageattn_hip_window.h for a call of at most 32 rows: one q-block per sequence)
 *
 * len_b = clamp(kv_lens[b], 0, max_pages * page_size), g = q_fold, the M = T * g <= 32 rows are T tokens, row r is token
 * t = r / g, and off_b = len_b - T.
 *
 *  1. Allowed keys.  Row r attends exactly the keys max(0, t + off_b - window + 1) <= j <= t + off_b.  A row without a key, and
 *     every row of a sequence without keys, gets o = 0 and lse = -inf, with or without sinks.
 *  2. Split ranges.  lo = max(off_b - window + 1, 0), hi = min((M - 1) / g + off_b, len_b - 1).  hi < 0: the sequence has no key.
 *     Otherwise its tiles are [tlo, thi] = [lo >> 6, hi >> 6], nt = thi - tlo + 1, tps = ceil(nt / S), and split s owns the tiles
 *     [tlo + s * tps, min(tlo + (s + 1) * tps, thi + 1)): point 2 of sageattn_hip_window.h.  A workgroup whose range is empty
 *     returns at once.
 *  3. Sinks.  sinks is fp32 [Hq] of the UN-folded view (in folded row t * g + i of KV head hk, head hk * g + i) or NULL, in the
 *     units of the returned LSE.  It is applied once, behind the correction q . km: lse' = logaddexp(lse, sink_h), o' = o *
 *     exp(lse - lse'), one rounding to the output type -- point 3 of sageattn_hip_window.h.  sinks != NULL with lse == NULL is
 *     SAGE_ERR_INVALID_ARGUMENT.
 *  4. Addresses.  No table entry below max(off_b - window + 1, 0) / page_size and none at or beyond ceil(len_b / page_size) is
 *     used to form an address.  Rows at or beyond len_b influence nothing, as in point 5 of sageattn_hip_decode.h (the FP8 V^T
 *     image with the exception stated there).
 *  5. Bit identity.  o and lse have the bits of sage_attn_fusedq_pv_*_splitkv_paged_window(causal = 1, q_fold = g) on the same
 *     arguments for every num_splits in 1 .. 16, every window, every length and every page size: the kernel does the arithmetic
 *     of that kernel's first wave in that wave's order, rows >= M keeping the limits of their row index on both sides, because
 *     the lazy rescale is decided over all 32 rows.  So with window >= max_pages * page_size and sinks == NULL they have the
 *     bits of sage_attn_fusedq_pv_*_decode_paged, and the one-launch path of num_splits == 1 has the bits of the two-launch
 *     path: a caller cannot tell them apart except by time and workspace.
 *
 * THE LAUNCHES
 *
 * num_splits == 1: ONE launch.  workspace may be NULL and workspace_bytes 0; nothing of it is touched.  The epilogue of the
 * attention kernel does what the merge does for one split on the values it holds, in the merge's order -- the natural-log LSE,
 * the correction (kept in a register: nothing is parked in lse), the sink term, one rounding of the output -- and a workgroup
 * of a sequence without keys stores its zeros and -inf.  With lse == NULL nothing is stored for it and km is not read.
 * num_splits > 1: two launches, the attention kernel over (b, h, split) with its fp32 partials in the workspace
 * (sage_splitkv_workspace_bytes) and the merge of sage_attn_fusedq_pv_*_splitkv_paged_window, unchanged.
 *
 * window is one int >= 1 for the call (window < 1: SAGE_ERR_INVALID_ARGUMENT); a value beyond max_pages * page_size means that
 * capacity.  M > 32: SAGE_ERR_UNSUPPORTED (use sage_attn_fusedq_pv_*_splitkv_paged_window).  D is 64 or 128, qk_gran per warp or
 * per thread, P.V fp16, bf16 or fp8, page_size 64, 128 or 256.
 *
 * NOT BUILT: the FP4 paged cache (it has no windowed four-wave form); the ragged and shared-prefix decode forms; a finish
 * inside the launch for num_splits > 1 (it needs an order between workgroups) or in sage_attn_fusedq_pv_*_decode_paged; more
 * than 16 splits; more than 32 rows; a window per sequence.
 */
#ifndef SAGEATTN_HIP_DECODE_WINDOW_H
#define SAGEATTN_HIP_DECODE_WINDOW_H

#include "sageattn_hip_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sage_attn_fusedq_pv_f16_decode_paged, its arguments in its order, then window and sinks (fp32 [Hq], 4-byte aligned, or NULL). */
int sage_attn_fusedq_pv_f16_decode_paged_window(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                const sage_tensor* v_pool, int v_dtype, const sage_tensor* o, int o_dtype,
                                                const float* k_scale_pool, const void* km, float* lse, int B, int Hq, int Hk,
                                                int M, int D, int qk_gran, int warpq, float sm_scale,
                                                const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                                int num_pages, const int32_t* kv_lens, int num_splits, int q_fold,
                                                void* workspace, size_t workspace_bytes, sage_stream_t stream, int window,
                                                const float* sinks);

/* ... with FP8 P.V, as sage_attn_fusedq_pv_f8_decode_paged */
int sage_attn_fusedq_pv_f8_decode_paged_window(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                               const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
                                               const float* k_scale_pool, const void* km, const float* v_scale, float* lse,
                                               int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq, float sm_scale,
                                               const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                               int num_pages, const int32_t* kv_lens, int num_splits, int q_fold,
                                               void* workspace, size_t workspace_bytes, sage_stream_t stream, int window,
                                               const float* sinks);

#ifdef __cplusplus
}
#endif

#endif /* SAGEATTN_HIP_DECODE_WINDOW_H */
