/*
 * sageattn_hip_decode.h -- extension of the C ABI (sageattn_hip_paged.h): DECODE attention on the paged cache, one wave per
 * split.  The split-KV kernels attend 128 query rows per workgroup with four waves of 32 rows; a decode step folded by its GQA
 * group has 4 .. 32 rows, and three of the four waves then work for rows nobody stores.  The two entry points here run a
 * kernel shaped for at most 32 query rows -- a workgroup is ONE wave and one split of one (sequence, head) -- on the pools, the
 * block table, the workspace (sage_splitkv_workspace_bytes) and the merge of sage_attn_fusedq_pv_*_splitkv_paged.  Nothing
 * dispatches to them implicitly.  Same conventions: device pointers, every argument is checked before any launch and a call
 * that returns an argument status has enqueued nothing.
 *
 * THE RULE
 *
 * len_b = clamp(kv_lens[b], 0, max_pages * page_size), g = q_fold, the M = T * g <= 32 rows are T tokens, row r is token
 * t = r / g, and off_b = len_b - T.
 *
 *  1. Always bottom-right causal: row r attends exactly the keys 0 <= j <= t + off_b.  For T = 1 that is every valid key.  A row
 *     with t + off_b < 0, and every row of a sequence without keys, gets o = 0 and lse = -inf.
 *  2. Split ranges, the count of non-empty splits, the frozen statistics of the cache, the workspace layout and the merge are
 *     those of sage_attn_fusedq_pv_*_splitkv_paged with causal = 1: split s of a batch with ntk_b = ceil(len_b / 64) tiles owns
 *     the tiles [s * tps_b, min((s + 1) * tps_b, ntk_b)), tps_b = ceil(ntk_b / S); a workgroup whose range is empty, or lies
 *     beyond the key bound of the last row, returns at once and stores nothing.  The merge launch is that entry's, unchanged.
 *  3. Bit identity.  o and lse have the bits of sage_attn_fusedq_pv_*_splitkv_paged(causal = 1, q_fold = g) on the same
 *     arguments, for every num_splits in 1 .. 16, every length and every page size.  The Q scale groups of the fused quantizer
 *     are per 32 rows, so wave 0 of that kernel depends on no other wave, and the kernel here does that wave's arithmetic in
 *     that wave's order: the S MFMAs, the dequantisation, the running maximum, the lazy rescale, the row sums (those on the
 *     matrix pipe at head_dim 64 with FP16 P.V included), the packing of P, the order of the P.V accumulation, the normalised
 *     fp32 partial and the raw base-2 LSE.  The correction q . km is parked in the caller's lse by split 0 only.
 *  4. Rows at or beyond M are the zero rows of the fused quantizer (their loads take the last row's bytes); they are never
 *     stored.
 *  5. Rows at or beyond len_b of the last page, NaN included, influence nothing: the descriptors of the batch's last K tile and
 *     16-bit V tile end at row len_b - 1, and tiles behind the last one are never copied.  The FP8 V^T image is the exception
 *     the paged entries share: a token is a COLUMN of it, which a descriptor cannot cut, so inside the batch's last 64-token
 *     block the kernel relies on the cache's own invariant that the append writes zeros into the columns at or beyond len_b
 *     (sageattn_hip_paged.h); their P is exactly 0, and 0 * 0 adds nothing.  Table entries at or beyond
 *     ceil(len_b / page_size) are not read.
 *
 * M > 32: SAGE_ERR_UNSUPPORTED (use sage_attn_fusedq_pv_*_splitkv_paged).  D is 64 or 128, qk_gran per warp or per thread,
 * P.V fp16, bf16 or fp8, page_size 64, 128 or 256, as there.
 *
 * The paged MXFP4 V cache has its own entry: sageattn_hip_decode_fp4.h.
 *
 * The window and sink forms, and with one split the merge inside the attention launch: sageattn_hip_decode_window.h.
 *
 * NOT BUILT: the contiguous caches; the ragged and shared-prefix forms; more than 16 splits; more than 32 rows; a merge inside
 * the attention launch of the two entries here.
 */
#ifndef SAGEATTN_HIP_DECODE_H
#define SAGEATTN_HIP_DECODE_H

#include "sageattn_hip_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sage_attn_fusedq_pv_f16_splitkv_paged without `causal`, its arguments in its order.  Two launches: attention over
 * (b, h, split) with one wave each, merge. */
int sage_attn_fusedq_pv_f16_decode_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                         const sage_tensor* v_pool, int v_dtype, const sage_tensor* o, int o_dtype,
                                         const float* k_scale_pool, const void* km, float* lse, int B, int Hq, int Hk, int M,
                                         int D, int qk_gran, int warpq, float sm_scale, const int32_t* block_table,
                                         int64_t table_stride, int max_pages, int page_size, int num_pages,
                                         const int32_t* kv_lens, int num_splits, int q_fold, void* workspace,
                                         size_t workspace_bytes, sage_stream_t stream);

/* ... with FP8 P.V, as sage_attn_fusedq_pv_f8_splitkv_paged */
int sage_attn_fusedq_pv_f8_decode_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                        const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
                                        const float* k_scale_pool, const void* km, const float* v_scale, float* lse, int B,
                                        int Hq, int Hk, int M, int D, int qk_gran, int warpq, float sm_scale,
                                        const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                        int num_pages, const int32_t* kv_lens, int num_splits, int q_fold, void* workspace,
                                        size_t workspace_bytes, sage_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGEATTN_HIP_DECODE_H */
