// Decode attention on the paged KV cache, one wave per split (the rule: include/sageattn_hip_decode.h).
//
// The split-KV kernels run the loop of sage_attn_body.h: a 256-thread workgroup whose four waves stage a 64-key tile together
// and attend 32 of the q-block's 128 rows each.  A decode step folded by its GQA group has 4 .. 32 rows: three of the four
// waves then read every fragment, issue every MFMA and take every exponential for rows nobody stores.
// attn_i8_decode_paged_kernel is a kernel of its own text for at most 32 query rows:
//
//  * A workgroup is ONE wave and one split of one (sequence, head): grid = B * Hq * S, splits of a head neighbours.
//  * The wave owns a private ring of kDecodeRing = 2 K slots and 2 V slots in LDS and fills it itself by LDS-DMA -- the copy
//    helper and the swizzles of the shared body, D / 16 copies of 64 x 16 bytes per K tile, D / 16 (FP8) or D / 8 (16-bit) per V
//    tile.  Iteration j issues K(j + 2) into the slot S(j) was computed from and V(j + 1) into the slot P(j - 1).V(j - 1) read,
//    computes S(j + 1) beside the softmax and P.V of tile j, and orders the ring with counted vmcnt waits alone: the copies a
//    wave issued are the only vector-memory operations of its loop, they complete in order, and nobody else writes its LDS.
//    There is no barrier in this kernel.  Two slots: 48 KiB at head_dim 128 with 16-bit P.V (3 workgroups in a CU's 160 KiB),
//    32 KiB with FP8 P.V (5), half of either at head_dim 64.
//  * Page ids come through the scalar cache an iteration ahead (page(j + 3) is requested in iteration j and first used in
//    iteration j + 1); every tile copy goes through a descriptor of its own with a 64-bit base, and the descriptor of the
//    batch's last tile ends at row len_b - 1, exactly as in the PAGED body.
//  * The arithmetic is that of wave 0 of attn_i8_splitkv_causal_paged_kernel, operation for operation in that wave's order (the
//    file is compiled with contraction off like the body): the fused Q quantizer on 32 rows, the S MFMAs on the biased
//    accumulator, dequantisation, the running maximum, the lazy rescale decided by a ballot over all 32 rows (rows >= M
//    included: they are zero rows with the limit of their row index, as there), the row sums (on the matrix pipe for FP16 P.V
//    at head_dim 64), P packing, the P.V accumulation order, the normalised fp32 partial and the raw base-2 LSE.  Only the
//    placement of the instructions is this kernel's own.  The merge is splitkv_merge_kernel<.., CAUSAL = true>, unchanged.
//
// attn_i8_decode_paged_v4_kernel (the rule: include/sageattn_hip_decode_fp4.h) is the same text, sage_attn_decode_body.h, on the
// paged MXFP4 V cache, with the bits of attn_i8_splitkv_causal_paged_v4_kernel.  What is its own is marked PV_FP4 there: V never
// touches LDS.  In the image the A fragment of lane (r, hh) for channel block dt is 16 contiguous bytes of the pool -- chunk hh
// of the 32-byte tile row of channel r + 32 * dt -- and in a one-wave workgroup no other wave wants them, so the lane loads its
// D / 32 fragments and its scale word of tile j + 1 straight into registers, behind the last P.V MFMA of tile j.  The ring is
// the K ring alone (16 KiB at head_dim 128), and the loads stand in the K copies' order of counted waits: NK copies, D / 32
// fragment loads and one scale load per tile.
#include <climits>
#include "../../include/sageattn_hip_decode.h"
#include "../../include/sageattn_hip_decode_fp4.h"
#include "sage_attn_launch.h"

namespace sage {

// The wave is one text for both kernels (sage_attn_decode_body.h), included INTO each as the shared attention body is: as a
// __forceinline__ device template hipcc allocated every register of the existing twelve instantiations anew.
template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
__global__ __launch_bounds__(64) void attn_i8_decode_paged_kernel(const AttnParams p) {
  constexpr bool PV_FP4 = false;
#define SAGE_ATTN_DECODE_BODY_OF_KERNEL
#include "sage_attn_decode_body.h"
#undef SAGE_ATTN_DECODE_BODY_OF_KERNEL
}

// ... on the paged MXFP4 V cache: P.V on the e2m1 image out of registers, P and everything before it as the FP8 mode
template <int D, bool KTHREAD>
__global__ __launch_bounds__(64) void attn_i8_decode_paged_v4_kernel(const AttnParams p) {
  constexpr bool V_BF16 = false, PV_FP8 = true, PV_FP4 = true;
#define SAGE_ATTN_DECODE_BODY_OF_KERNEL
#include "sage_attn_decode_body.h"
#undef SAGE_ATTN_DECODE_BODY_OF_KERNEL
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int launch_decode_attn(const AttnCall& c, bool pv_fp4, hipStream_t st, int grid) {
  if (pv_fp4)
    return by_dim(c.D, [&](auto d) {
      return by_flag(c.kthread, [&](auto k) {
        constexpr int D = decltype(d)::value;
        constexpr size_t smem = decode_lds_bytes(D, true, true);
        void (*kern)(const AttnParams) = attn_i8_decode_paged_v4_kernel<D, decltype(k)::value>;
        if (!allow_lds((const void*)kern, smem)) return (int)SAGE_ERR_LAUNCH;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64), smem, st, c.p);
        return launch_status();
      });
    });
  return by_dim(c.D, [&](auto d) {
    return by_flag(c.pv_fp8, [&](auto fp8) {
      constexpr int D = decltype(d)::value;
      constexpr bool PV_FP8 = decltype(fp8)::value;
      constexpr size_t smem = decode_lds_bytes(D, PV_FP8);
      return by_flag(c.kthread, [&](auto k) {
        return by_flag(c.v_bf16, [&](auto v) {
          void (*kern)(const AttnParams) =
              attn_i8_decode_paged_kernel<D, decltype(k)::value, !PV_FP8 && decltype(v)::value, PV_FP8>;
          if (!allow_lds((const void*)kern, smem)) return (int)SAGE_ERR_LAUNCH;
          hipLaunchKernelGGL(kern, dim3(grid), dim3(64), smem, st, c.p);
          return launch_status();
        });
      });
    });
  });
}

// What is the decode form's own is checked here, the rest as sage_attn_fusedq_pv_*_splitkv_paged(causal = 1) checks it; nothing
// is enqueued before every check has passed.  pv_fp4: v is the image pool and v_scale carries the scale pool's bytes, as in
// sage_attn_fusedq_pv_f4_splitkv_paged.
static int decode_entry(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                        const sage_tensor* o, int o_dtype, const float* k_scale, const void* km, bool pv_fp8,
                        bool pv_fp4, const float* v_scale, float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq,
                        float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                        int num_pages, const int32_t* kv_lens, int num_splits, int q_fold, void* workspace,
                        size_t workspace_bytes, sage_stream_t stream) {
  if (pv_fp8 && !v_scale) return SAGE_ERR_INVALID_ARGUMENT;
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  if (page_size != 64 && page_size != 128 && page_size != 256) return SAGE_ERR_INVALID_ARGUMENT;
  if (!block_table || ((uintptr_t)block_table & 3) || !kv_lens || max_pages < 1 || num_pages < 1 || table_stride < max_pages ||
      table_stride > INT_MAX)
    return SAGE_ERR_INVALID_ARGUMENT;
  if ((int64_t)max_pages * page_size > INT_MAX) return SAGE_ERR_TOO_LARGE;
  // a row of the image holds the page's tiles side by side: narrower, a tile's loads would reach into the next channel
  if (pv_fp4 && v && v->stride_n < page_size / 2) return SAGE_ERR_INVALID_ARGUMENT;
  if (M > kDecodeMaxRows) return SAGE_ERR_UNSUPPORTED;  // (more rows: sage_attn_fusedq_pv_*_splitkv_paged)
  AttnArgs a;
  a.q = q; a.q_dtype = q_dtype; a.k8 = k8; a.v = v; a.v_dtype = v_dtype; a.o = o; a.o_dtype = o_dtype; a.k_scale = k_scale;
  a.km = km; a.v_scale = v_scale; a.pv_fp8 = pv_fp8; a.lse = lse;
  a.B = B; a.Hq = Hq; a.Hk = Hk; a.M = M; a.N = max_pages * page_size; a.D = D; a.qk_gran = qk_gran; a.blkq = 128; a.warpq = warpq;
  a.sm_scale = sm_scale;
  a.split_kv = true; a.split_kv_lens = kv_lens; a.num_splits = num_splits; a.split_workspace = workspace;
  a.split_workspace_bytes = workspace_bytes;
  a.split_causal = true; a.q_fold = q_fold;
  a.paged = true; a.block_table = block_table; a.table_stride = (int)table_stride; a.page_size = page_size;
  AttnCall c;
  if (const int s = attn_check(c, a)) return s;
  if ((int64_t)B * Hq * num_splits > INT_MAX) return SAGE_ERR_TOO_LARGE;
  if (pv_fp4) c.p.v_tile_bytes = 32;  // a tile of the image is 32 bytes of every channel row
  const int s = launch_decode_attn(c, pv_fp4, (hipStream_t)stream, B * Hq * num_splits);
  return s ? s : launch_splitkv_merge(c, (hipStream_t)stream);
}

}  // namespace sage

using namespace sage;

extern "C" int sage_attn_fusedq_pv_f16_decode_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                    const sage_tensor* v_pool, int v_dtype, const sage_tensor* o, int o_dtype,
                                                    const float* k_scale_pool, const void* km, float* lse, int B, int Hq,
                                                    int Hk, int M, int D, int qk_gran, int warpq, float sm_scale,
                                                    const int32_t* block_table, int64_t table_stride, int max_pages,
                                                    int page_size, int num_pages, const int32_t* kv_lens, int num_splits,
                                                    int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  return decode_entry(q, q_dtype, k8_pool, v_pool, v_dtype, o, o_dtype, k_scale_pool, km, false, false, nullptr, lse, B, Hq, Hk, M, D,
                      qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages, kv_lens, num_splits,
                      q_fold, workspace, workspace_bytes, stream);
}

extern "C" int sage_attn_fusedq_pv_f8_decode_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                   const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
                                                   const float* k_scale_pool, const void* km, const float* v_scale, float* lse,
                                                   int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq, float sm_scale,
                                                   const int32_t* block_table, int64_t table_stride, int max_pages,
                                                   int page_size, int num_pages, const int32_t* kv_lens, int num_splits,
                                                   int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  return decode_entry(q, q_dtype, k8_pool, v8_pool, SAGE_F16, o, o_dtype, k_scale_pool, km, true, false, v_scale, lse, B, Hq, Hk, M, D,
                      qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages, kv_lens, num_splits,
                      q_fold, workspace, workspace_bytes, stream);
}

extern "C" int sage_attn_fusedq_pv_f4_decode_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                   const sage_tensor* v_img_pool, const sage_tensor* o, int o_dtype,
                                                   const float* k_scale_pool, const void* km, const uint8_t* v_img_scale_pool,
                                                   float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq,
                                                   float sm_scale, const int32_t* block_table, int64_t table_stride,
                                                   int max_pages, int page_size, int num_pages, const int32_t* kv_lens,
                                                   int num_splits, int q_fold, void* workspace, size_t workspace_bytes,
                                                   sage_stream_t stream) {
  return decode_entry(q, q_dtype, k8_pool, v_img_pool, SAGE_F16, o, o_dtype, k_scale_pool, km, true, true,
                      reinterpret_cast<const float*>(v_img_scale_pool), lse, B, Hq, Hk, M, D, qk_gran, warpq, sm_scale,
                      block_table, table_stride, max_pages, page_size, num_pages, kv_lens, num_splits, q_fold, workspace,
                      workspace_bytes, stream);
}
