/*
 * sageattn_hip_ragged.h -- extension of the C ABI (sageattn_hip.h, sageattn_hip_paged.h): causal split-KV attention on the paged
 * cache for a MIXED batch, one call per layer.  The queries are packed as a serving engine with continuous batching keeps
 * them, q [total_tokens, Hq, D] with cu_seqlens_q [B + 1]: a prefill chunk of 2048 tokens beside 63 decode sequences of one
 * token each is 2111 rows, not 64 x 2048.  Same conventions: device pointers, element strides, the caller owns every buffer,
 * every argument is checked before any launch and a call that returns an argument status has enqueued nothing.
 *
 * OPERANDS
 *
 * The pools, block_table [B, table_stride >= max_pages], kv_lens [B], km [B,Hk,D] and v_scale [B,Hk,D] exactly as
 * sageattn_hip_paged.h describes them.
 * q is [total_tokens, Hq, D]: q->stride_n is the stride of a TOKEN, q->stride_h that of a head, q->stride_b is not read; any
 * strides that are multiples of 8 elements are read in place (a view into a fused QKV projection output).  o likewise
 * (multiples of 4 elements), lse fp32 [total_tokens, Hq] contiguous or NULL.
 * cu_seqlens_q int32 [B + 1] on the device, read there only.  T_b = cu[b + 1] - cu[b].
 * q_fold = g is 1 or Hq / Hk.  With g = Hq / Hk the g query heads of a KV head become query rows, token-major, as in
 * sage_attn_fusedq_pv_*_splitkv_causal: row t * g + i of KV head hk is q[token t, head hk * g + i].  The kernel's addressing
 * does the fold; nothing is copied.
 *
 * THE RULE
 *
 *  1. len_b = clamp(kv_lens[b], 0, max_pages * page_size).  Token t of sequence b, 0 <= t < T_b, attends the keys
 *     0 <= j <= t + len_b - T_b and nothing later: the T_b tokens are the LAST positions of the sequence's len_b keys.  A token
 *     whose bound is negative gives o = 0 and lse = -inf; so does every token of a sequence without keys.
 *  2. For every sequence b the rows of its tokens in o and lse are BIT-IDENTICAL to
 *     sage_attn_fusedq_pv_*_splitkv_paged(causal = 1, q_fold = g, num_splits = S) on that sequence alone: B' = 1, Hq' = Hq / g,
 *     M' = T_b * g, q_b = q[cu[b] : cu[b + 1]] folded by hand into [1, Hq / g, T_b * g, D], row b of the table, kv_lens[b],
 *     km[b], v_scale[b].  So the 128-row q-blocks, the 32-row scale groups of the fused Q quantizer and its per-thread groups
 *     restart at each sequence, and the split ranges are the per-sequence tps_b = ceil(ntk_b / S) of the existing rule.
 *  3. The work list.  sage_ragged_q_plan writes int32 pairs (b, qb), one per 128-row q-block that exists -- qb <
 *     ceil(T_b * g / 128) -- in sequence order, into n_items = total_tokens * g / 128 + B slots (integer division; an upper
 *     bound the host knows from shapes); unused slots hold b = -1.  One workgroup, a scan, no atomics: deterministic.  The
 *     list depends on cu_seqlens_q, total_tokens and g only, so one plan serves every layer of a step.
 *  4. The attention grid is n_items x (Hq / g) x S workgroups, the split fastest and the items of one head neighbours.  A
 *     workgroup reads its pair with one scalar load and leaves before any barrier on b < 0.  Its partial results go to a
 *     workspace indexed by packed row, fp32 [S, Hq / g, total_tokens * g, D] and the base-2 LSEs [S, Hq / g, total_tokens * g].
 *  5. The merge walks the same list: the count of splits of a q-block from T_b and len_b as the merge of the split-KV entry
 *     points derives it, that merge's arithmetic in split order, o stored at [token, hk * g + i, :] and lse at
 *     [token, hk * g + i]; q-blocks where no split ran get the defined zeros and -inf.
 *  6. A sequence with T_b = 0 has no list entry: nothing of o or lse is written for it and nothing of its table row is read.
 *     Rows at or beyond len_b, table entries at or beyond ceil(len_b / page_size) and pages the sequence does not name
 *     influence nothing, exactly as items 4 to 6 of sageattn_hip_paged.h say.
 *  7. Everything is read on the device only: {plan; attention} captures into one HIP graph and a replay follows what
 *     cu_seqlens_q, kv_lens and the table hold then, for the same B and total_tokens.
 *
 * Preconditions, stated and not checked: cu[0] = 0, cu is non-decreasing, cu[B] = total_tokens, and those of
 * sageattn_hip_paged.h.  A cu_seqlens_q that breaks them gives undefined values but no load or store outside the buffers: the
 * plan never writes more than n_items entries, and the kernels clamp cu[b] to [0, total_tokens] and T_b to
 * [0, total_tokens - cu[b]], so that no token index reaches total_tokens.
 *
 * num_splits is one count for the whole call.  The Python layer's default, splitkv_num_splits(1, Hq / g, 128 * n_items,
 * max_pages * page_size), is the existing function on the work list's size: a guess that nobody has measured on a mixed batch.
 *
 * NOT BUILT: ragged queries on the FP4 paged cache (sageattn_hip_paged_fp4.h) and on the contiguous caches; a non-causal ragged
 * form; packed new rows for sage_kv_cache_append_rows_paged, which still takes [B, Hk, T, D] (sage_kv_cache_append_paged
 * already serves ragged growth through start_lens / kv_lens); a split count per sequence; ordering the work list by cost; the
 * shared-prefix operator (sageattn_hip_prefix.h) with ragged suffix queries.
 */
#ifndef SAGEATTN_HIP_RAGGED_H
#define SAGEATTN_HIP_RAGGED_H

#include "sageattn_hip_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The work list of rule 3: one launch of one workgroup.
 *   cu_seqlens_q   int32 [B + 1], 4-byte aligned
 *   items          int32 [n_items][2], 8-byte aligned;  n_items must be total_tokens * q_fold / 128 + B
 * B, total_tokens, q_fold < 1, a NULL or misaligned pointer, another n_items -> SAGE_ERR_INVALID_ARGUMENT; total_tokens * q_fold
 * beyond INT_MAX or more than INT_MAX / 256 items -> SAGE_ERR_TOO_LARGE. */
int sage_ragged_q_plan(const int32_t* cu_seqlens_q, int B, int total_tokens, int q_fold, int32_t* items, int n_items,
                       sage_stream_t stream);

/* Bytes of the workspace of a ragged call (rule 4): num_splits * Hq * total_tokens * (D + 1) * 4, which is
 * sage_splitkv_workspace_bytes(1, Hq, total_tokens, D, num_splits).  0 for a size below 1 or num_splits outside 1..16. */
size_t sage_ragged_workspace_bytes(int total_tokens, int Hq, int D, int num_splits);

/* Ragged causal split-KV attention by the rule above: two launches (attention over the list, merge).  The pools, the table's
 * arguments and kv_lens are those of sage_attn_fusedq_pv_f16_splitkv_paged.
 *   q, o            [total_tokens, Hq, D] as described above
 *   lse             fp32 [total_tokens, Hq] or NULL
 *   items, n_items  the list sage_ragged_q_plan wrote for (cu_seqlens_q, total_tokens, q_fold)
 *   num_splits      1..16
 *   q_fold          1 or Hq / Hk
 *   workspace       16-byte aligned, sage_ragged_workspace_bytes(total_tokens, Hq, D, num_splits) bytes
 * Checked before any launch: total_tokens < 1, a q_fold that is neither 1 nor Hq / Hk, a NULL or misaligned cu_seqlens_q or
 * items, n_items != total_tokens * q_fold / 128 + B, a workspace that is too small -> SAGE_ERR_INVALID_ARGUMENT;
 * total_tokens * q_fold, the item count or either grid beyond its int range -> SAGE_ERR_TOO_LARGE; everything else as
 * sage_attn_fusedq_pv_f16_splitkv_paged with causal != 0. */
int sage_attn_fusedq_pv_f16_splitkv_paged_ragged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                 const sage_tensor* v_pool, int v_dtype, const sage_tensor* o, int o_dtype,
                                                 const float* k_scale_pool, const void* km, float* lse, int B, int Hq, int Hk,
                                                 int total_tokens, int D, int qk_gran, int warpq, float sm_scale,
                                                 const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                                 int num_pages, const int32_t* kv_lens, const int32_t* cu_seqlens_q,
                                                 const int32_t* items, int n_items, int num_splits, int q_fold, void* workspace,
                                                 size_t workspace_bytes, sage_stream_t stream);

/* ... with FP8 P.V: v8_pool is the V^T image per page, v_scale fp32 [B,Hk,D] the frozen scales, 16-byte aligned. */
int sage_attn_fusedq_pv_f8_splitkv_paged_ragged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
                                                const float* k_scale_pool, const void* km, const float* v_scale, float* lse,
                                                int B, int Hq, int Hk, int total_tokens, int D, int qk_gran, int warpq,
                                                float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages,
                                                int page_size, int num_pages, const int32_t* kv_lens,
                                                const int32_t* cu_seqlens_q, const int32_t* items, int n_items, int num_splits,
                                                int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGEATTN_HIP_RAGGED_H */
