// Paged split-KV attention on the MXFP4 V image of the KV cache (the rule: include/sageattn_hip_paged_fp4.h): the two halves
// that were built to compose.  The body is sage_attn_body.h with SPLITKV = true, PAGED = true and its third P.V mode, PV_FP4:
// the split's range of logical 64-key tiles, the page lookup an iteration ahead and the per-tile descriptors are those of
// sage_attn_splitkv_paged.hip; the [D][32]-byte V tiles, their swizzle, the scale register and the MFMA with an e2m1 A operand
// those of sage_attn_splitkv_v4.hip.  What exists only here:
//   * the V tile copy out of a page of the image pool [P,Hk,D,32*tpp]: a descriptor of the tile's own, base = pool + page *
//     page stride + hk * head stride + (tile in page) * 32, (D - 1) * row stride + 32 bytes long.  Every wave copies the same
//     number of chunks (head_dim 64: waves 2 and 3 repeat those of waves 0 and 1), which the counted waits of the ring need;
//   * the scale bytes out of a page of the scale pool [P,Hk,tpp,2*D]: the per-lane load issued behind the last P.V MFMA of
//     tile j takes its scalar base from the page of tile j + 1, which the loop holds an iteration ahead.
// A scale group lies inside one 64-key tile and nothing of V is frozen, so a page's bytes depend on its own rows only: o and
// lse are bit-identical to sage_attn_fusedq_pv_f4_splitkv[_causal] on the gathered cache.  The merge is that of
// sage_attn_splitkv.hip.
//
// Kernels of their own names in a file of their own, as every other twin of the body: the other instantiations keep their
// code and their registers.  Only what is dispatched is instantiated: 4 waves, fused Q, per-thread and per-warp scales.
#include <climits>
#include "sage_attn_launch.h"
#include "../../include/sageattn_hip_paged_fp4.h"

namespace sage {

#define SAGE_ATTN_BODY_PV_FP4
template <int D, bool KTHREAD>
// (register budget as the FP8 mode: head_dim 64 is held to three waves per SIMD)
__global__ __launch_bounds__(256, D == 64 ? 3 : 2)
void attn_i8_splitkv_paged_v4_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool V_BF16 = false, PV_FP8 = true;
  constexpr bool CAUSAL = false, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true, PAGED = true;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

template <int D, bool KTHREAD>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2)
void attn_i8_splitkv_causal_paged_v4_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool V_BF16 = false, PV_FP8 = true;
  constexpr bool CAUSAL = true, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true, PAGED = true;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}
#undef SAGE_ATTN_BODY_PV_FP4

// LDS of a launch: the four-slot ring of the FP8 mode with V tiles of half the size (as sage_attn_splitkv_v4.hip)
constexpr size_t attn_v4_lds_bytes(int D) { return (size_t)attn_ring_slots(D, 4, true) * (64 * D + 32 * D); }

}  // namespace sage

using namespace sage;

// The entry point of both forms.  What is the table's own and the pools' own is checked here, the rest by attn_check on the
// pools as for the paged FP8 form (stride_b of k8 / v_img is the stride of a page; its window check counts 64 bytes per tile
// and row where the image has 32: a (page, head) slice it refuses is at most twice the size of one that fits).  The scale
// pool travels in the word of v_scale; its strides follow from Hk and the page size.  Nothing is enqueued before every check
// has passed.
extern "C" int sage_attn_fusedq_pv_f4_splitkv_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                    const sage_tensor* v_img_pool, const sage_tensor* o, int o_dtype,
                                                    const float* k_scale_pool, const void* km, const uint8_t* v_img_scale_pool,
                                                    float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq,
                                                    float sm_scale, const int32_t* block_table, int64_t table_stride,
                                                    int max_pages, int page_size, int num_pages, const int32_t* kv_lens,
                                                    int num_splits, int causal, int q_fold, void* workspace,
                                                    size_t workspace_bytes, sage_stream_t stream) {
  if (!v_img_scale_pool) return SAGE_ERR_INVALID_ARGUMENT;
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  if (page_size != 64 && page_size != 128 && page_size != 256) return SAGE_ERR_INVALID_ARGUMENT;
  if (!block_table || ((uintptr_t)block_table & 3) || !kv_lens || max_pages < 1 || num_pages < 1 || table_stride < max_pages ||
      table_stride > INT_MAX)
    return SAGE_ERR_INVALID_ARGUMENT;
  if ((int64_t)max_pages * page_size > INT_MAX) return SAGE_ERR_TOO_LARGE;
  // a row of the image holds the page's tiles side by side: narrower, a tile's descriptor would reach into the next channel
  if (v_img_pool && v_img_pool->stride_n < page_size / 2) return SAGE_ERR_INVALID_ARGUMENT;
  AttnArgs a;
  a.q = q; a.q_dtype = q_dtype; a.k8 = k8_pool; a.v = v_img_pool; a.v_dtype = SAGE_F16; a.o = o; a.o_dtype = o_dtype;
  a.k_scale = k_scale_pool; a.km = km; a.v_scale = reinterpret_cast<const float*>(v_img_scale_pool); a.pv_fp8 = true; a.lse = lse;
  a.B = B; a.Hq = Hq; a.Hk = Hk; a.M = M; a.N = max_pages * page_size; a.D = D; a.qk_gran = qk_gran; a.blkq = 128; a.warpq = warpq;
  a.sm_scale = sm_scale;
  a.split_kv = true; a.split_kv_lens = kv_lens; a.num_splits = num_splits; a.split_workspace = workspace;
  a.split_workspace_bytes = workspace_bytes;
  a.split_causal = causal != 0; a.q_fold = causal ? q_fold : 1;
  a.paged = true; a.block_table = block_table; a.table_stride = (int)table_stride; a.page_size = page_size;
  AttnCall c;
  if (const int s = attn_check(c, a)) return s;
  c.p.v_tile_bytes = 32;  // a tile of the image is 32 bytes of every channel row
  const int grid = c.p.nqb * c.p.Hq * c.p.B * c.p.num_splits;
  const hipStream_t st = (hipStream_t)stream;
  const bool is_causal = causal != 0;
  const int s = by_dim(c.D, [&](auto d) {
    return by_flag(c.kthread, [&](auto k) {
      constexpr int DD = decltype(d)::value;
      constexpr bool KT = decltype(k)::value;
      constexpr size_t smem = attn_v4_lds_bytes(DD);
      void (*kern)(const AttnParams) =
          is_causal ? attn_i8_splitkv_causal_paged_v4_kernel<DD, KT> : attn_i8_splitkv_paged_v4_kernel<DD, KT>;
      if (!allow_lds((const void*)kern, smem)) return (int)SAGE_ERR_LAUNCH;
      hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, c.p);
      return launch_status();
    });
  });
  return s ? s : launch_splitkv_merge(c, st);
}
