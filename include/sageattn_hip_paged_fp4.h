/*
 * sageattn_hip_paged_fp4.h -- extension of the C ABI (sageattn_hip.h, sageattn_hip_paged.h, sageattn_hip_fp4.h): the MXFP4
 * image of V of sageattn_hip_fp4.h for the PAGED quantized KV cache of sageattn_hip_paged.h.  Same conventions: device
 * pointers, element strides, the caller owns every buffer, every argument is checked before the launch and a call that
 * returns an argument status has enqueued nothing.
 *
 * A serving engine keeps KV in fixed-size pages named by a block table.  Without this header such a caller reaches the FP4
 * P.V path only by gathering every sequence into a padded tensor on every step, which costs more than the bytes FP4 saves.
 * The two halves were built to compose: a scale group of the image lies inside one 64-key tile, like the scale groups of K,
 * and nothing of V is frozen -- there are no V coefficients -- so a page's image bytes and scale bytes depend on the page's own
 * rows only.  Paging is an addressing change, not a numerical one.
 *
 * LAYOUT
 *
 * k_pool, v_pool (fp16 / bf16), k8_pool (INT8) and k_scale_pool are those of sageattn_hip_paged.h, page_size 64, 128 or 256
 * keys, tpp = page_size / 64 tiles per page; block_table, kv_lens, start_lens and km [B,H,D] as there.  The V state:
 *   img_pool    uint8 [P,H,D,32*tpp]: a sage_tensor whose stride_b is the stride of a page and stride_n the stride of a
 *               channel d (bytes, >= 32*tpp); the 32 bytes of tile ti of the page start at 32*ti of a channel's row.  Nibble
 *               order inside a tile: sageattn_hip_fp4.h
 *   scale_pool  uint8 [P,H,tpp,2*D] contiguous: the 2*D e8m0 bytes of tile ti of (page, head), ordered [hh][c % 32][c / 32]
 * Both shapes are the same for either layout of the fp16 pools.  Logical tile t of batch b is tile t % tpp of page
 * block_table[b, t / tpp].
 *
 * THE RULE
 *
 * Let ref be the contiguous cache of sageattn_hip_fp4.h (sage_kv_cache_append_v4 and the K half of sageattn_hip_kvcache.h) on
 * the padded tensors gathered from the pages in table order, with the same km and lengths.  After the first append from 0,
 * and after any sequence of appends:
 *
 *  1. Every valid tile equals ref's, bit for bit: its INT8 rows < len_b, its K scales, its image bytes and its scale bytes,
 *     with the zero nibbles of the rows [len_b, 64 * ceil(len_b / 64)) and the 127 bytes of a group without a valid row.
 *  2. sage_kv_cache_append_paged_v4 follows the rule of sage_kv_cache_append_v4 in LOGICAL tile indices: it touches the tiles
 *     t0_b .. ceil(len_b / 64) - 1, t0_b = floor(min(start_b, len_b - 1) / 64); start_b >= len_b (no new rows, or a
 *     rollback) re-quantizes exactly the ragged tile; len_b == 0 touches nothing and reads nothing of the table row.  No byte
 *     of an untouched tile and no byte of a page the sequence does not name is written.  Rows at or beyond len_b are never
 *     loaded: a clamped row index lies in [0, len_b) and therefore in a named page.
 *  3. sage_attn_fusedq_pv_f4_splitkv_paged returns o and lse bit-identical to sage_attn_fusedq_pv_f4_splitkv[_causal] on ref
 *     for every num_splits, causal with q_fold included: the split ranges follow len_b in 64-key tiles and do not depend on
 *     page_size.  Therefore lse equals that of the paged FP8 cache on the same K.  A sequence without keys gives o = 0 and
 *     lse = -inf.
 *  4. No table entry at or beyond ceil(len_b / page_size) is read, for the image or for the scale bytes: every read-ahead is
 *     clamped to the last tile the workgroup needs.  No page the sequence does not name is read.  The ragged last tile needs
 *     no shorter descriptor: the append wrote its zero nibbles.
 *  5. The table and the lengths are read on the device only: {append; attention} captures into one HIP graph, and a replay
 *     reads what the tensors hold then.
 *  6. Pools of any size are valid: a tile's address is formed in 64 bits on the scalar unit, and only a (page, head) slice goes
 *     through a 32-bit offset; one that does not fit the 2^31 window is SAGE_ERR_TOO_LARGE.
 *
 * Preconditions, stated and not checked: those of sageattn_hip_paged.h (valid entries in [0, P); the valid pages of different
 * batches distinct; rows < start_b unchanged; len_b - min(start_b, len_b) <= max_new).  A tile no append has written must
 * decode to zeros if it can become valid later without an append from its first row: allocate img_pool as zeros and
 * scale_pool as 127.
 *
 * The causal and the non-causal form share ONE attention entry point (`causal`, `q_fold`), as in sageattn_hip_paged.h: the
 * header holds two entry points.
 *
 * NOT BUILT: an FP4 image for the cache without fp16 pools of sageattn_hip_paged_rows.h (a scale group is a maximum over 32
 * tokens, so a step that adds rows to a group needs the group's earlier rows: an fp16 V tail per sequence); the shared-prefix
 * operator of sageattn_hip_prefix.h on this cache; page sizes below 64; FP4 for P, Q or K.
 */
#ifndef SAGEATTN_HIP_PAGED_FP4_H
#define SAGEATTN_HIP_PAGED_FP4_H

#include "sageattn_hip_paged.h"
#include "sageattn_hip_fp4.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sage_kv_cache_append_paged with the MXFP4 image as its V half: (K tile slots + V unit slots, H, B) workgroups, one launch;
 * a slot looks its page up in the table.  The arguments of sage_kv_cache_append_paged with img_pool / scale_pool in the place
 * of v8_pool / v_coef; v_pool, img_pool and scale_pool are required.
 * Checked before the launch: page_size not 64 / 128 / 256, a NULL or misaligned table, image (16 bytes, strides multiples of
 * 16, stride_n >= page_size / 2) or scale pool (16 bytes), max_pages < 1, num_pages < 1, table_stride < max_pages, and
 * everything sage_kv_cache_append_v4 checks -> SAGE_ERR_INVALID_ARGUMENT; D not 64 or 128 -> SAGE_ERR_UNSUPPORTED_HEAD_DIM;
 * max_pages * page_size beyond INT_MAX, or a (page, head) slice of the image beyond the 32-bit window -> SAGE_ERR_TOO_LARGE. */
int sage_kv_cache_append_paged_v4(const sage_tensor* k_pool, const sage_tensor* v_pool, int dtype, int B, int H, int D,
                                  const void* km, const sage_tensor* k8_pool, float* k_scale_pool, int gran, int rounding,
                                  const sage_tensor* img_pool, uint8_t* scale_pool, const int32_t* block_table,
                                  int64_t table_stride, int max_pages, int page_size, int num_pages, const int32_t* start_lens,
                                  const int32_t* kv_lens, int max_new, sage_stream_t stream);

/* Split-KV attention on the paged image: the arguments, checks and statuses of sage_attn_fusedq_pv_f8_splitkv_paged with
 * v_img_pool / v_img_scale_pool in the place of v8_pool / v_scale (NULL or misaligned, or a row of the image narrower than
 * page_size / 2 bytes: SAGE_ERR_INVALID_ARGUMENT); causal != 0: the causal form with q_fold (not read otherwise).  kv_lens is
 * required.  workspace: sage_splitkv_workspace_bytes(B, Hq, M, D, num_splits). */
int sage_attn_fusedq_pv_f4_splitkv_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                         const sage_tensor* v_img_pool, const sage_tensor* o, int o_dtype,
                                         const float* k_scale_pool, const void* km, const uint8_t* v_img_scale_pool, float* lse,
                                         int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq, float sm_scale,
                                         const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                         int num_pages, const int32_t* kv_lens, int num_splits, int causal, int q_fold,
                                         void* workspace, size_t workspace_bytes, sage_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGEATTN_HIP_PAGED_FP4_H */
