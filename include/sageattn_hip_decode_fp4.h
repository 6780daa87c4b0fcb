/*
 * sageattn_hip_decode_fp4.h -- extension of the C ABI (sageattn_hip_decode.h, sageattn_hip_paged_fp4.h): DECODE attention on the
 * paged MXFP4 V cache, one wave per split.  The cache with the fewest bytes per key -- at head_dim 128 128 B of INT8 K, 64 B
 * of e2m1 V and 4 scale bytes per key and KV head, 196 B against 256 B (FP8) and 384 B (FP16) -- was the one cache the one-wave
 * kernel of sageattn_hip_decode.h could not serve.  The entry point here runs attn_i8_decode_paged_v4_kernel on the pools, the
 * block table, the workspace (sage_splitkv_workspace_bytes) and the merge of sage_attn_fusedq_pv_f4_splitkv_paged.  Nothing
 * dispatches to it implicitly.  Same conventions: device pointers, every argument is checked before any launch and a call that
 * returns an argument status has enqueued nothing.
 *
 * THE RULE is that of sageattn_hip_decode.h with the V half of sageattn_hip_paged_fp4.h.
 *
 * len_b = clamp(kv_lens[b], 0, max_pages * page_size), g = q_fold, the M = T * g <= 32 rows are T tokens, row r is token
 * t = r / g, and off_b = len_b - T.
 *
 *  1. Always bottom-right causal: row r attends exactly the keys 0 <= j <= t + off_b.  A row with t + off_b < 0, and every row
 *     of a sequence without keys, gets o = 0 and lse = -inf.
 *  2. Split ranges, the count of non-empty splits, the workspace layout and the merge launch are those of
 *     sage_attn_fusedq_pv_f4_splitkv_paged with causal = 1, unchanged.
 *  3. Bit identity.  o and lse have the bits of sage_attn_fusedq_pv_f4_splitkv_paged(causal = 1, q_fold = g) on the same
 *     arguments, for every num_splits in 1 .. 16, every length and every page size.  The kernel does the arithmetic of that
 *     kernel's first wave in that wave's order: the fused Q quantizer on 32 rows, the biased S MFMAs, the dequantisation, the
 *     running maximum, the lazy rescale by ballot over all 32 rows, P in e4m3 with the FP8 mode's exponent offset and its row
 *     sums; P.V on v_mfma_scale_f32_32x32x64_f8f6f4 with A = e2m1 (cbsz 4), the A scale byte dt of the lane's scale word and
 *     the B scale 2^0; an epilogue without a V-scale multiply that stores the normalised fp32 partial and the raw base-2 LSE.
 *     Therefore lse equals sage_attn_fusedq_pv_f8_decode_paged on the FP8 cache over the same K.
 *  4. V does not pass through LDS.  In the image the A fragment of lane (r, hh) for channel block dt is 16 contiguous bytes of
 *     the pool, chunk hh of the 32-byte tile row of channel r + 32 * dt (sageattn_hip_fp4.h), and a one-wave workgroup has no
 *     other wave that wants them: the lane loads its D / 32 fragments and its scale word a tile ahead, straight into registers.
 *     A tile's address is a 64-bit scalar base; only a (page, head) slice goes through a 32-bit lane offset.
 *  5. What influences nothing: rows at or beyond len_b, table entries at or beyond ceil(len_b / page_size), and pages the
 *     sequence does not name.  The K descriptor of the batch's last tile ends at row len_b - 1; the image relies on the zero
 *     nibbles the append wrote into the columns at or beyond len_b, as the paged FP4 entries do.  Every read-ahead -- page ids,
 *     K copies, image fragments, scale bytes -- stops at the last tile the workgroup needs.
 *
 * M > 32: SAGE_ERR_UNSUPPORTED (use sage_attn_fusedq_pv_f4_splitkv_paged).  D is 64 or 128, qk_gran per warp or per thread,
 * page_size 64, 128 or 256, as there.
 *
 * NOT BUILT: the contiguous FP4 cache; the ragged, window, sink and shared-prefix forms; an FP4 image for the cache without
 * fp16 pools; K fragments straight to registers; a third K slot; more than 16 splits; more than 32 rows; a merge inside the
 * attention launch; FP4 for P, Q or K.
 */
#ifndef SAGEATTN_HIP_DECODE_FP4_H
#define SAGEATTN_HIP_DECODE_FP4_H

#include "sageattn_hip_paged_fp4.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sage_attn_fusedq_pv_f4_splitkv_paged without `causal`, its arguments in its order.  Two launches: attention over
 * (b, h, split) with one wave each, merge. */
int sage_attn_fusedq_pv_f4_decode_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                        const sage_tensor* v_img_pool, const sage_tensor* o, int o_dtype,
                                        const float* k_scale_pool, const void* km, const uint8_t* v_img_scale_pool, float* lse,
                                        int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq, float sm_scale,
                                        const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                        int num_pages, const int32_t* kv_lens, int num_splits, int q_fold, void* workspace,
                                        size_t workspace_bytes, sage_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGEATTN_HIP_DECODE_FP4_H */
