/*
 * sageattn_hip_paged_rows.h -- extension of the C ABI (sageattn_hip.h, sageattn_hip_paged.h): the paged quantized KV cache of
 * sageattn_hip_paged.h WITHOUT fp16 / bf16 pools of the caller's.  The append takes the step's new K / V rows as arguments,
 * [B, H, T, D] as they leave the projection, and the cache owns every pool; of fp16 K it keeps the rows of the CURRENT 64-key
 * tile per sequence and head alone (k_tail), because a K scale group is a maximum over the rows of a tile and a new row can
 * move it.  Same conventions: device pointers, element strides, the caller owns every buffer, every argument is checked
 * before the launch and a call that returns an argument status has enqueued nothing.
 *
 * Bytes per cached key and KV head at head_dim 128: fp16 cache 512; sageattn_hip_paged.h 768.25 (FP8 P.V) / 640.25 (FP16
 * P.V), its fp16 pools included; this form 256.25 / 384.25, plus the tail: 2 * 64 * D elements per sequence and head.
 *
 * STATE
 *
 * k8_pool, k_scale_pool, km and, for FP8 P.V, v8_pool, v_scale, v_coef: as sageattn_hip_paged.h.  For FP16 / BF16 P.V: v_pool
 * [P, H, page_size, D] in the input dtype, which the append FILLS.  New: k_tail, the input dtype, [B, H, 2, 64, D] contiguous,
 * a ring of two tile slots: row r of a sequence lives in slot (r >> 6) & 1, row r & 63.  There is no fp16 K pool, and with FP8
 * P.V no fp16 V anywhere.
 *
 * THE RULE
 *
 * ref is the cache of sageattn_hip_paged.h over fp16 / bf16 pools into which the same rows were written, with the same block
 * table, lengths, granularity and frozen statistics.  Nothing numerical is new: the rule is bit-exactness against ref.
 *
 * Lengths, for batch b: s_b = clamp(start_lens[b]), len_b = clamp(kv_lens[b]), both to [0, max_pages * page_size];
 * n_b = max(len_b - s_b, 0); tl_b = (len_b - 1) >> 6; t0_b = min(s_b, len_b - 1) >> 6.  The touched tiles are t0_b .. tl_b.
 *
 *  1. K.  Logical K row s_b + i is k_new[b, :, i], i < n_b; the rows [64 * t0_b, min(s_b, len_b)) of tile t0_b come from the
 *     ring.  Every touched K tile -- its INT8 rows < len_b and its scales -- is bit-identical to the same tile of ref after the
 *     same call.  No byte of another tile is written and no byte of a page the sequence does not name.  len_b == 0 touches
 *     nothing.  Rows of k_new / v_new at i >= n_b are never loaded: NaN there changes nothing.
 *  2. V, FP8 P.V.  The bytes of tokens [s_b, len_b) in the V^T image are ref's (the same conversion, clamped to +-448 under the
 *     frozen v_coef), the bytes of tokens [len_b, 64 * ceil(len_b / 64)) of the last block are zero, and the bytes of tokens
 *     < min(s_b, len_b) keep their values: V is quantized element by element under frozen coefficients and needs no tail.  Inside
 *     a block the image's token order is permuted and four consecutive tokens share a dword, so a block that holds older tokens
 *     is merged per byte.
 *     V, FP16 / BF16 P.V.  Rows [s_b, len_b) of v_new are copied into the named pages of v_pool; nothing else is written.
 *  3. The ring after the call: for every row r in [s_b, len_b) of tile tl_b or tl_b - 1, slot (r >> 6) & 1, row r & 63 holds
 *     the input row, bit for bit.  Rows of earlier tiles need not be written.  The ring of another (b, h) is not touched.
 *  4. The table and the lengths are read on the device only.
 *
 * Preconditions, stated and not checked:
 *  - those of sageattn_hip_paged.h about the table;
 *  - n_b <= T;
 *  - t0_b >= hi_b - 1, hi_b the largest tile index any earlier call (since the statistics were frozen) wrote rows of.  This
 *    admits rolling back up to 64 rejected speculative rows across a tile boundary and "overwrite and extend" in one call
 *    (s_b below the old length); it excludes two rollbacks in a row past two tile boundaries: a ring of two slots then no
 *    longer holds the tile the sequence fell back into.
 *
 * NOT BUILT: the same for the contiguous cache of sageattn_hip_kvcache.h; moving frozen statistics without preparing again.
 * A prefix the sequences share is a sequence of its own: sageattn_hip_prefix.h.
 */
#ifndef SAGEATTN_HIP_PAGED_ROWS_H
#define SAGEATTN_HIP_PAGED_ROWS_H

#include "sageattn_hip_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Append rows to a paged cache by the rule above, in ONE launch of (K tile slots + V unit slots, H, B) workgroups: the grid and
 * slot arithmetic of sage_kv_cache_append_paged with max_new = T.
 *   k_new, v_new     fp16 / bf16 (dtype) [B,H,T,D] descriptors, T >= 1: last dim contiguous, data 16-byte aligned, strides
 *                    multiples of 8 elements (a strided view of a fused QKV projection is valid)
 *   km               [B,H,D] in the input dtype, 16-byte aligned (read only)
 *   k_tail           [B,H,2,64,D] contiguous in the input dtype, 16-byte aligned (read and written)
 *   k8_pool, k_scale_pool, gran, rounding    as sage_kv_cache_append_paged
 *   v_pool           fp16 / bf16 [P,H,page_size,D], FILLED (FP16 / BF16 P.V), or NULL
 *   v8_pool          the V^T image per page (stride_n = stride of d), or NULL;  v_coef fp32 [B,H,2,D], required with it
 *                    exactly ONE of v_pool / v8_pool is given
 *   block_table ... num_pages, start_lens, kv_lens    as sage_kv_cache_append_paged
 * Checked before the launch, each fault with the status sage_kv_cache_append_paged gives it; T < 1, a NULL or misaligned k_tail,
 * both or neither of v_pool / v8_pool, v8_pool without v_coef -> SAGE_ERR_INVALID_ARGUMENT; a (page, head) slice of k8_pool,
 * v_pool or v8_pool beyond the 32-bit window -> SAGE_ERR_TOO_LARGE. */
int sage_kv_cache_append_rows_paged(const sage_tensor* k_new, const sage_tensor* v_new, int dtype, int B, int H, int T, int D,
                                    const void* km, void* k_tail, const sage_tensor* k8_pool, float* k_scale_pool, int gran,
                                    int rounding, const sage_tensor* v_pool, const sage_tensor* v8_pool, const float* v_coef,
                                    const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                    int num_pages, const int32_t* start_lens, const int32_t* kv_lens, sage_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGEATTN_HIP_PAGED_ROWS_H */
