/*
 * sageattn_hip_paged.h -- extension of the C ABI (sageattn_hip.h, sageattn_hip_kvcache.h): the persistent quantized KV cache
 * of sageattn_hip_kvcache.h stored in fixed-size PAGES of one pool, addressed through a per-sequence block table, as serving
 * engines keep their caches.  Same conventions: device pointers, element strides, the caller owns every buffer, every
 * argument is checked before the launch and a call that returns an argument status has enqueued nothing.
 *
 * LAYOUT
 *
 * A pool is a sage_tensor whose stride_b is the stride of a PAGE: k_pool, v_pool (fp16 / bf16) and k8_pool (INT8) are
 * [P, H, page_size, D], v8_pool (FP8 P.V only) is the V^T image per page, [P, H, D, page_size] with stride_n the stride of
 * d: its 64-token blocks are 64 bytes apart along the last dim, in the token order of the contiguous image.  k_scale_pool is
 * fp32 [P, H, (page_size / 64) * g] contiguous, g = 4 (per_thread) or 1 (per_block).  page_size is 64, 128 or 256 keys: the
 * scale groups of K and the blocks of the V^T image are 64-key tiles, so a page is a whole number of them.
 * block_table is int32 [B, table_stride >= max_pages]: entries [0, ceil(len_b / page_size)) of row b are page ids in [0, P),
 * len_b = clamp(kv_lens[b], 0, N), N = max_pages * page_size the logical capacity.  Logical 64-key tile t of batch b is tile
 * t % (page_size / 64) of page block_table[b, t / (page_size / 64)].  km [B,H,D], v_scale [B,H,D] and v_coef [B,H,2,D] stay
 * per SEQUENCE, as in sageattn_hip_kvcache.h.
 *
 * THE RULE
 *
 * Let gather(x)[b] be the padded [H, N, D] tensor made of row b's pages in table order, and ref the contiguous cache of
 * sageattn_hip_kvcache.h on gather(k_pool), gather(v_pool) with the same km, v_coef and lengths.
 *
 * Paging is an addressing change, not a numerical one: a K tile's INT8 rows and scales depend on the tile's own rows and on
 * km, a block of the V^T image on its own rows and on v_coef, and both statistics are per sequence.
 *
 *  1. Statistics.  km, v_scale and v_coef are the caller's, frozen per sequence.  The Python layer (SagePagedKVCache.prepare)
 *     obtains them by gathering the valid prefix of every sequence ONCE into a padded copy and running the length-aware
 *     pre-pass on it: exactly ref's.  That cost is paid once per sequence or serving slot; it is not the hot path.  It then
 *     writes every valid page with one sage_kv_cache_append_paged from start = 0.
 *  2. Append.  sage_kv_cache_append_paged follows the rule of sage_kv_cache_append in LOGICAL tile indices: the touched
 *     tiles t0_b .. ceil(len_b / 64) - 1, t0_b = floor(min(start_b, len_b - 1) / 64); the start_b >= len_b / rollback case;
 *     max_new; the +-448 clamp.  Every touched tile -- its INT8 rows < len_b, its scales, for FP8 its V^T block with the zero
 *     bytes of the columns [len_b, 64 * ceil(len_b / 64)) -- is bit-identical to the same tile of ref after the same appends.
 *     No byte of a tile that is not touched is written and no byte of a page the sequence does not name.  (At head_dim 64 a V
 *     workgroup holds two 64-token blocks, with 64-key pages two pages of the sequence: the whole block below an odd t0_b is
 *     rewritten with the same bytes, as in the contiguous form.)
 *  3. Attention.  sage_attn_fusedq_pv_{f16,f8}_splitkv_paged return o and lse bit-identical to
 *     sage_attn_fusedq_pv_{f16,f8}_splitkv[_causal] on ref with the same kv_lens, num_splits (and q_fold).  The split ranges
 *     follow len_b in 64-key tiles and do not depend on page_size; num_splits = 1 runs the paged kernel with one split.  The
 *     workspace is that of sage_splitkv_workspace_bytes, and the merge kernel is the one of the contiguous form.
 *  4. Nothing outside the valid range has any influence.  Rows at or beyond len_b inside the last page are never loaded by
 *     the append and reach the attention kernel's LDS as zeros, NaN in the fp16 / bf16 pools included: the descriptor of the
 *     sequence's last tile ends with row len_b - 1.  Table entries at an index >= ceil(len_b / page_size) are never used to
 *     form an address, and the row is never read at an index >= max_pages: every read-ahead is clamped to the index of the
 *     last tile the workgroup needs.  Pages that no valid entry names are never touched.  A batch without keys gives o = 0
 *     and lse = -inf, and nothing of its table row is read.
 *  5. The table and the lengths are read on the device only: no host synchronisation, {append; attention} captures into one
 *     HIP graph, and a replay reads the table and the lengths the tensors hold then.
 *  6. 64-bit page addressing.  Pools of any size are valid: the address of a tile is formed in 64 bits on the scalar unit
 *     (pool + page * page stride + head * head stride + tile * tile bytes) and becomes words 0-1 of a buffer descriptor of
 *     the tile's own; only the bytes inside one (page, head) slice go through a 32-bit offset, and a slice that does not fit
 *     the 2^31 window is SAGE_ERR_TOO_LARGE.
 *
 * Preconditions, stated and not checked (checking them would need a host read):
 *  - valid entries lie in [0, P);
 *  - the valid pages of different batches are distinct: km and the V scale are per sequence;
 *  - the rows < start_b are unchanged since they were quantized; len_b - min(start_b, len_b) <= max_new.
 *
 * A cache that owns every pool and keeps no fp16 K pool: sageattn_hip_paged_rows.h.
 *
 * NOT BUILT: page sizes below 64 (a 16-key page cannot hold a scale group); paged forms of the dense, kvlen and block-sparse
 * operators; moving frozen statistics without preparing again.  Pages are not shared between sequences -- the frozen
 * statistics are per sequence; a prefix the sequences share is a sequence of its own: sageattn_hip_prefix.h.
 */
#ifndef SAGEATTN_HIP_PAGED_H
#define SAGEATTN_HIP_PAGED_H

#include "sageattn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Extend the prepared operands of a paged cache by the rule above, in ONE launch of (K tile slots + V unit slots, H, B)
 * workgroups, the grid and slot arithmetic of sage_kv_cache_append in logical tiles; a slot looks its page up in the table.
 *   k_pool, v_pool   the caller's fp16 / bf16 pools (dtype); v_pool may be NULL when v8_pool is
 *   km               [B,H,D] in k's dtype, 16-byte aligned (read only)
 *   k8_pool          INT8, shaped as k_pool;  k_scale_pool fp32 [P,H,(page_size/64)*g] contiguous
 *   gran, rounding   as sage_kv_cache_append
 *   v8_pool          the V^T image per page (stride_n = stride of d), or NULL: no V half;  v_coef fp32 [B,H,2,D], required with it
 *   block_table      int32 [B, table_stride], 4-byte aligned;  max_pages >= 1 entries of a row are the sequence's
 *   page_size        64, 128 or 256;  num_pages = P >= 1
 *   start_lens,      int32 [B], 4-byte aligned
 *   kv_lens
 *   max_new          >= 1: the most rows any batch gains in this call
 * Checked before the launch: page_size not 64 / 128 / 256, a NULL or misaligned table, max_pages < 1, num_pages < 1,
 * table_stride < max_pages, and everything sage_kv_cache_append checks -> SAGE_ERR_INVALID_ARGUMENT; D not 64 or 128 ->
 * SAGE_ERR_UNSUPPORTED_HEAD_DIM; max_pages * page_size beyond INT_MAX -> SAGE_ERR_TOO_LARGE. */
int sage_kv_cache_append_paged(const sage_tensor* k_pool, const sage_tensor* v_pool, int dtype, int B, int H, int D,
                               const void* km, const sage_tensor* k8_pool, float* k_scale_pool, int gran, int rounding,
                               const sage_tensor* v8_pool, const float* v_coef, const int32_t* block_table,
                               int64_t table_stride, int max_pages, int page_size, int num_pages, const int32_t* start_lens,
                               const int32_t* kv_lens, int max_new, sage_stream_t stream);

/* Split-KV attention on a paged cache: sage_attn_fusedq_pv_f16_splitkv (causal != 0: ..._splitkv_causal with q_fold; q_fold
 * is not read otherwise) with k8, v and k_scale as pools and N = max_pages * page_size.  kv_lens is required.  There is no
 * v_mean.  workspace: sage_splitkv_workspace_bytes(B, Hq, M, D, num_splits).
 * Checked before any launch: the table arguments as above, a NULL kv_lens -> SAGE_ERR_INVALID_ARGUMENT; a (page, head) slice
 * of k8_pool or v_pool / v8_pool beyond the 32-bit window -> SAGE_ERR_TOO_LARGE; everything else as the contiguous entries. */
int sage_attn_fusedq_pv_f16_splitkv_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                          const sage_tensor* v_pool, int v_dtype, const sage_tensor* o, int o_dtype,
                                          const float* k_scale_pool, const void* km, float* lse, int B, int Hq, int Hk, int M,
                                          int D, int qk_gran, int warpq, float sm_scale, const int32_t* block_table,
                                          int64_t table_stride, int max_pages, int page_size, int num_pages,
                                          const int32_t* kv_lens, int num_splits, int causal, int q_fold, void* workspace,
                                          size_t workspace_bytes, sage_stream_t stream);

/* ... with FP8 P.V: v8_pool is the V^T image per page, v_scale fp32 [B,Hk,D] the frozen per-sequence scale. */
int sage_attn_fusedq_pv_f8_splitkv_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                         const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
                                         const float* k_scale_pool, const void* km, const float* v_scale, float* lse, int B,
                                         int Hq, int Hk, int M, int D, int qk_gran, int warpq, float sm_scale,
                                         const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                         int num_pages, const int32_t* kv_lens, int num_splits, int causal, int q_fold,
                                         void* workspace, size_t workspace_bytes, sage_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGEATTN_HIP_PAGED_H */
