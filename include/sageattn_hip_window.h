/*
 * sageattn_hip_window.h -- extension of the C ABI (sageattn_hip_paged.h, sageattn_hip_ragged.h): SLIDING-WINDOW attention and
 * SINK LOGITS on the paged cache.  Mistral and Gemma 2/3 attend the last `window` keys only; gpt-oss does so in every other layer
 * and adds a learned logit per query head to every softmax denominator.  The four entry points are the causal paged split-KV
 * entry and its ragged form with two more arguments, `window` and `sinks`; operands, layouts, q_fold, the work list and the
 * workspaces (sage_splitkv_workspace_bytes, sage_ragged_workspace_bytes) are the parents'.  Same conventions: device pointers,
 * every argument is checked before any launch and a call that returns an argument status has enqueued nothing.
 *
 * THE RULE
 *
 * len_b = clamp(kv_lens[b], 0, max_pages * page_size), g = q_fold, row r is token t = r / g, T_b the tokens of sequence b (M / g,
 * or cu[b + 1] - cu[b]) and off_b = len_b - T_b, as in the causal operators.
 *
 *  1. Allowed keys.  Row r attends exactly the keys max(0, t + off_b - window + 1) <= j <= t + off_b, j < len_b.  A row with
 *     t + off_b < 0, and every row of a sequence without keys, gets o = 0 and lse = -inf, with or without sinks.
 *  2. Ranges, per 128-row q-block (restarting at each sequence in the ragged form).  tok0 and tok1 are the tokens of the block's
 *     first row and of its last row < M; lo = max(tok0 + off_b - window + 1, 0), hi = min(tok1 + off_b, len_b - 1).  hi < 0: the
 *     block has no key.  Otherwise its tiles are [tlo, thi] = [lo >> 6, hi >> 6], nt = thi - tlo + 1, tps = ceil(nt / S), and split
 *     s owns the tiles [tlo + s * tps, min(tlo + (s + 1) * tps, thi + 1)).  A workgroup whose range is empty returns before any
 *     barrier; the merge derives the same count per q-block, ceil(nt / tps), and reads no slot beyond it.  The merge is
 *     deterministic and in split order.
 *  3. Sinks.  sinks is fp32 [Hq] (the query heads of the UN-folded view) or NULL.  The value is in the units of the returned LSE
 *     -- the natural log of the scaled logits -- and belongs to the query head: in a folded row t * g + i of KV head hk, head
 *     hk * g + i.  It is applied once, in the merge, behind the correction q . km: lse' = logaddexp(lse, sink_h), o' = o *
 *     exp(lse - lse'), and o' is rounded once to the output type.  NULL runs the same kernels without the term.  The merge
 *     needs the corrected LSE of every row for it: sinks != NULL with lse == NULL is SAGE_ERR_INVALID_ARGUMENT.
 *  4. Addresses.  For sequence b no table entry below max(off_b - window + 1, 0) / page_size (integer division) and none at or
 *     beyond ceil(len_b / page_size) is used to form an address, and no tile below a workgroup's tlo is copied: an engine may
 *     free the pages that have left the window, whatever their table entries hold then.
 *  5. Bit anchors.  With window >= len_b and num_splits = 1, o and lse have the bits of sage_attn_fusedq_pv_*_splitkv_paged(causal =
 *     1, num_splits = 1); with one q-block per sequence, for every num_splits.  For each sequence the ragged form has the bits of
 *     the non-ragged window entry on that sequence alone.
 *
 * window is one int >= 1 for the call (window < 1: SAGE_ERR_INVALID_ARGUMENT); a value beyond max_pages * page_size means that
 * capacity.  num_splits is one count for the call.
 *
 * NOT BUILT: windows on the contiguous caches, on the FP4 paged cache and in the shared-prefix operator; a non-causal or dense
 * windowed form; sink TOKENS (StreamingLLM's pinned first keys); a window per sequence.
 */
#ifndef SAGEATTN_HIP_WINDOW_H
#define SAGEATTN_HIP_WINDOW_H

#include "sageattn_hip_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sage_attn_fusedq_pv_f16_splitkv_paged, its arguments in its order, then window and sinks (4-byte aligned).  causal must be
 * non-zero: there is no non-causal windowed form (SAGE_ERR_UNSUPPORTED).  Two launches: attention over (b, h, q-block, split),
 * merge. */
int sage_attn_fusedq_pv_f16_splitkv_paged_window(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                 const sage_tensor* v_pool, int v_dtype, const sage_tensor* o, int o_dtype,
                                                 const float* k_scale_pool, const void* km, float* lse, int B, int Hq, int Hk,
                                                 int M, int D, int qk_gran, int warpq, float sm_scale,
                                                 const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                                 int num_pages, const int32_t* kv_lens, int num_splits, int causal,
                                                 int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream,
                                                 int window, const float* sinks);

/* ... with FP8 P.V, as sage_attn_fusedq_pv_f8_splitkv_paged */
int sage_attn_fusedq_pv_f8_splitkv_paged_window(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
                                                const float* k_scale_pool, const void* km, const float* v_scale, float* lse,
                                                int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq, float sm_scale,
                                                const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                                int num_pages, const int32_t* kv_lens, int num_splits, int causal,
                                                int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream,
                                                int window, const float* sinks);

/* sage_attn_fusedq_pv_f16_splitkv_paged_ragged, its arguments in its order, then window and sinks fp32 [Hq]. */
int sage_attn_fusedq_pv_f16_splitkv_paged_ragged_window(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                        const sage_tensor* v_pool, int v_dtype, const sage_tensor* o,
                                                        int o_dtype, const float* k_scale_pool, const void* km, float* lse,
                                                        int B, int Hq, int Hk, int total_tokens, int D, int qk_gran, int warpq,
                                                        float sm_scale, const int32_t* block_table, int64_t table_stride,
                                                        int max_pages, int page_size, int num_pages, const int32_t* kv_lens,
                                                        const int32_t* cu_seqlens_q, const int32_t* items, int n_items,
                                                        int num_splits, int q_fold, void* workspace, size_t workspace_bytes,
                                                        sage_stream_t stream, int window, const float* sinks);

/* ... with FP8 P.V, as sage_attn_fusedq_pv_f8_splitkv_paged_ragged */
int sage_attn_fusedq_pv_f8_splitkv_paged_ragged_window(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                       const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
                                                       const float* k_scale_pool, const void* km, const float* v_scale,
                                                       float* lse, int B, int Hq, int Hk, int total_tokens, int D, int qk_gran,
                                                       int warpq, float sm_scale, const int32_t* block_table,
                                                       int64_t table_stride, int max_pages, int page_size, int num_pages,
                                                       const int32_t* kv_lens, const int32_t* cu_seqlens_q, const int32_t* items,
                                                       int n_items, int num_splits, int q_fold, void* workspace,
                                                       size_t workspace_bytes, sage_stream_t stream, int window,
                                                       const float* sinks);

#ifdef __cplusplus
}
#endif

#endif /* SAGEATTN_HIP_WINDOW_H */
