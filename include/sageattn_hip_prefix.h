/*
 * sageattn_hip_prefix.h -- extension of the C ABI (sageattn_hip.h, sageattn_hip_paged.h): split-KV attention on a paged cache
 * whose sequences share a PREFIX -- a system prompt, a few-shot header -- that is stored once.  Same conventions: device
 * pointers, element strides, the caller owns every buffer, every argument is checked before any launch and a call that
 * returns an argument status has enqueued nothing.
 *
 * Pages cannot simply be named by several block-table rows: the smoothing vector km and the FP8 V scale are per sequence
 * (sageattn_hip_paged.h), so a page's quantized bytes belong to one sequence.  Here the prefix IS a sequence of its own, with
 * its own frozen km_p and v_scale_p, each suffix keeps its own, and a row's attention over prefix plus suffix is the
 * log-sum-exp merge of two partial attentions.  The prefix pass folds the B sequences' query rows into the rows of one
 * "batch", so the prefix K / V leave HBM once for the whole batch: B * (Np + Ns) key rows become Np + B * Ns.
 *
 * OPERANDS
 *
 * One set of pools, exactly as sageattn_hip_paged.h describes: k8_pool, k_scale_pool, and v_pool or v8_pool.
 * The prefix sequence: prefix_table int32 [max_prefix_pages]; prefix_len int32 [1] on the device; km_p [1,Hk,D]; FP8 P.V
 * only: v_scale_p fp32 [1,Hk,D].  Lp = clamp(prefix_len[0], 0, max_prefix_pages * page_size).
 * B suffix sequences: block_table [B, table_stride >= max_pages], kv_lens [B], km [B,Hk,D], v_scale [B,Hk,D].  They count and
 * address the SUFFIX keys only: len_b = clamp(kv_lens[b], 0, max_pages * page_size).
 * q is [B,Hq,M,D] as the causal paged operator takes it: q_fold = g divides M, row r is token r / g, and the M / g tokens are
 * the last positions of the suffix.
 *
 * THE RULE
 *
 * Row (b, h, m) attends every prefix key [0, Lp) and the suffix keys that sage_attn_fusedq_pv_*_splitkv_causal gives it at
 * len_b.
 *
 *  1. Segment results.  Prefix: attn_i8_splitkv_paged_kernel (non-causal) with B' = 1, Hq' = Hq, M' = B * M on the view
 *     q_p[0, h, b * M + m] = q[b, h, m], prefix_splits = Sp splits, km_p and v_scale_p.  Suffix: the causal paged kernel on q
 *     with num_splits = Ss and q_fold.  Both launches get an LSE scratch pointer, so split 0 of each parks its q . km_seg.  The
 *     partial slots are, bit for bit, those sage_attn_fusedq_pv_*_splitkv_paged writes for the same arguments.
 *  2. Per-segment merge, for x in {p, s}.  count_x is derived exactly as the merge of the split-KV entry points derives it:
 *     non-causal with B = 1 for p, the causal count of the row's q-block for s.  mx_x, sum_x and acc_x are that merge's
 *     arithmetic, in split order, with the same selects; no slot at or beyond count_x is read.  Then, in fp32 and with
 *     contraction off,
 *         o_x = acc_x * (1 / sum_x),      L_x = (mx_x + log2f(sum_x)) / 1.44269504f + corr_x * sm_scale,
 *     the operations of that merge's LSE tail, and L_x = -inf where the segment has no key for the row.  The raw base-2 LSEs
 *     of the two kernels lack q . km_seg, which differs per segment: each correction enters its segment's weight BEFORE the
 *     segments are combined.
 *  3. Combine.  mx = max(L_p, L_s); w_x = expf(L_x - mx), dropped by a select where L_x = -inf;
 *         o = round_to_dtype((o_p * w_p + o_s * w_s) * (1 / (w_p + w_s))),      lse = mx + logf(w_p + w_s),
 *     summed in the order prefix, suffix.  A row without any key gives o = 0 and lse = -inf.  Where ONE segment alone has a
 *     key for the row, w = 1 and the combine is the identity on it: lse = L_x, and o is rounded from the product
 *     acc_x * (1 / sum_x) itself, as that segment's own merge rounds it, not from the fp32 o_x (for fp16 the merge's product and
 *     rounding are one instruction with one rounding; a detour through fp32 would round twice).
 *
 * Consequences:
 *  - When only one segment has keys for a row, the row has the BITS of the existing operator on that segment, o and
 *    (when requested) lse: Lp = 0 gives sage_attn_fusedq_pv_*_splitkv_paged (causal) on the suffixes, every len_b = 0 gives
 *    the un-folded non-causal call on the prefix with the folded q.
 *  - The prefix bytes in the pools depend on the prefix rows and the prefix statistics only: one prefix serves any batch.
 *  - Everything rule 4 of sageattn_hip_paged.h says about rows and table entries beyond the lengths holds for both tables.
 *  - Lengths and tables are read on the device only (rule 5 there): {append; attention} captures into one HIP graph.
 *
 * The folded q must be addressable with one row stride: q->stride_b == M * q->stride_n (NHD-contiguous q), or M == 1 (the
 * row stride is then stride_b); any other q is SAGE_ERR_UNSUPPORTED and the caller passes a copy.
 *
 * Preconditions, stated and not checked: those of sageattn_hip_paged.h for both tables, and the valid prefix pages are
 * distinct from every valid suffix page.
 *
 * NOT BUILT: more than one prefix per call, or trees of prefixes; one fused launch over both segments; the two attention
 * launches on two streams; prefix sharing for the contiguous cache of sageattn_hip_kvcache.h; moving frozen statistics without
 * preparing again.
 */
#ifndef SAGEATTN_HIP_PREFIX_H
#define SAGEATTN_HIP_PREFIX_H

#include "sageattn_hip_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of a shared-prefix call: the partial slots of the prefix pass,
 * sage_splitkv_workspace_bytes(1, Hq, B * M, D, prefix_splits), those of the suffix pass, sage_splitkv_workspace_bytes(B, Hq,
 * M, D, num_splits), and the two parked corrections, 2 * B * Hq * M * 4.  0 for a size below 1 or splits outside 1..16. */
size_t sage_prefix_workspace_bytes(int B, int Hq, int M, int D, int prefix_splits, int num_splits);

/* Shared-prefix attention by the rule above: three launches (prefix pass, suffix pass, merge).  The arguments up to kv_lens
 * are those of sage_attn_fusedq_pv_f16_splitkv_paged and describe the SUFFIXES; the suffix pass is always causal.
 *   prefix_table      int32 [max_prefix_pages], 4-byte aligned;  max_prefix_pages >= 1
 *   prefix_len        int32 [1], 4-byte aligned
 *   km_p              [1,Hk,D] in q's dtype, 16-byte aligned
 *   prefix_splits,    1..16 each
 *   num_splits
 *   q_fold            >= 1, divides M
 *   workspace         16-byte aligned, sage_prefix_workspace_bytes(B, Hq, M, D, prefix_splits, num_splits) bytes
 * Checked before any launch: a NULL or misaligned prefix_table or prefix_len, max_prefix_pages < 1, a workspace that is too
 * small -> SAGE_ERR_INVALID_ARGUMENT; a q whose folded view has no single row stride -> SAGE_ERR_UNSUPPORTED; B * M or
 * max_prefix_pages * page_size beyond INT_MAX -> SAGE_ERR_TOO_LARGE; everything else as sage_attn_fusedq_pv_f16_splitkv_paged
 * with causal != 0, for both segments. */
int sage_attn_fusedq_pv_f16_splitkv_paged_prefix(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                 const sage_tensor* v_pool, int v_dtype, const sage_tensor* o, int o_dtype,
                                                 const float* k_scale_pool, const void* km, float* lse, int B, int Hq, int Hk,
                                                 int M, int D, int qk_gran, int warpq, float sm_scale,
                                                 const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                                 int num_pages, const int32_t* kv_lens, const int32_t* prefix_table,
                                                 int max_prefix_pages, const int32_t* prefix_len, const void* km_p,
                                                 int prefix_splits, int num_splits, int q_fold, void* workspace,
                                                 size_t workspace_bytes, sage_stream_t stream);

/* ... with FP8 P.V: v8_pool is the V^T image per page, v_scale fp32 [B,Hk,D] the suffixes' frozen scales and v_scale_p fp32
 * [1,Hk,D] the prefix's, both 16-byte aligned. */
int sage_attn_fusedq_pv_f8_splitkv_paged_prefix(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
                                                const float* k_scale_pool, const void* km, const float* v_scale, float* lse,
                                                int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq, float sm_scale,
                                                const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                                int num_pages, const int32_t* kv_lens, const int32_t* prefix_table,
                                                int max_prefix_pages, const int32_t* prefix_len, const void* km_p,
                                                const float* v_scale_p, int prefix_splits, int num_splits, int q_fold,
                                                void* workspace, size_t workspace_bytes, sage_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGEATTN_HIP_PREFIX_H */
