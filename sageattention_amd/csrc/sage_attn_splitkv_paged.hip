// Paged split-KV attention (the rule: include/sageattn_hip_paged.h): attn_i8_splitkv_kernel (sage_attn_splitkv.hip) on a KV
// cache that is stored in fixed-size pages of one pool.  The body is sage_attn_body.h with SPLITKV = true, PAGED = true: the
// split's range of logical 64-key tiles is that of the contiguous kernel -- it follows len_b and does not know the page size --
// and only where a tile comes from changes: its page is looked up in the batch's block-table row (scalar cache, an iteration
// ahead) and the copy goes through a descriptor of the tile's own, whose 64-bit base may lie anywhere in the pool.  The fp32
// partial results and the merge (splitkv_merge_kernel, sage_attn_splitkv.hip) are those of the contiguous call.
//
// A kernel of its own name and a source file of its own, as every other twin: the build's guards match kernels by name, and
// the other instantiations keep their code and their registers.  The causal twin is sage_attn_splitkv_causal_paged.hip; the
// two entry points of both forms are here.
#include <climits>
#include "../../include/sageattn_hip_paged.h"
#include "sage_attn_launch.h"

namespace sage {

template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
// (register budget as attn_i8_kernel: head_dim 64 FP8 PV with 4 waves is held to three waves per SIMD)
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_splitkv_paged_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = false, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true, PAGED = true;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// the attention launch over (b, h, q-block, split) of a non-causal paged call
int launch_splitkv_paged_attn(const AttnCall& c, hipStream_t st) {
  return launch_4wave_kernel(c, st, c.p.nqb * c.p.Hq * c.p.B * c.p.num_splits, [](auto d, auto k, auto v, auto fp8) {
    return attn_i8_splitkv_paged_kernel<decltype(d)::value, decltype(k)::value, decltype(v)::value, decltype(fp8)::value>;
  });
}

// A paged entry point: what is its own is checked here, the rest by attn_check on the pools (stride_b of k8 / v is the stride
// of a page), then the launches of a split-KV call.  Nothing is enqueued before every check has passed.
static int splitkv_paged_entry(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                               const sage_tensor* o, int o_dtype, const float* k_scale, const void* km, bool pv_fp8,
                               const float* v_scale, float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq,
                               float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                               int num_pages, const int32_t* kv_lens, int num_splits, int causal, int q_fold, void* workspace,
                               size_t workspace_bytes, sage_stream_t stream) {
  if (pv_fp8 && !v_scale) return SAGE_ERR_INVALID_ARGUMENT;
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  if (page_size != 64 && page_size != 128 && page_size != 256) return SAGE_ERR_INVALID_ARGUMENT;
  if (!block_table || ((uintptr_t)block_table & 3) || !kv_lens || max_pages < 1 || num_pages < 1 || table_stride < max_pages ||
      table_stride > INT_MAX)
    return SAGE_ERR_INVALID_ARGUMENT;
  if ((int64_t)max_pages * page_size > INT_MAX) return SAGE_ERR_TOO_LARGE;
  AttnArgs a;
  a.q = q; a.q_dtype = q_dtype; a.k8 = k8; a.v = v; a.v_dtype = v_dtype; a.o = o; a.o_dtype = o_dtype; a.k_scale = k_scale;
  a.km = km; a.v_scale = v_scale; a.pv_fp8 = pv_fp8; a.lse = lse;
  a.B = B; a.Hq = Hq; a.Hk = Hk; a.M = M; a.N = max_pages * page_size; a.D = D; a.qk_gran = qk_gran; a.blkq = 128; a.warpq = warpq;
  a.sm_scale = sm_scale;
  a.split_kv = true; a.split_kv_lens = kv_lens; a.num_splits = num_splits; a.split_workspace = workspace;
  a.split_workspace_bytes = workspace_bytes;
  a.split_causal = causal != 0; a.q_fold = causal ? q_fold : 1;
  a.paged = true; a.block_table = block_table; a.table_stride = (int)table_stride; a.page_size = page_size;
  AttnCall c;
  if (const int s = attn_check(c, a)) return s;
  return attn_launch(c, (hipStream_t)stream);
}

}  // namespace sage

using namespace sage;

extern "C" int sage_attn_fusedq_pv_f16_splitkv_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                     const sage_tensor* v_pool, int v_dtype, const sage_tensor* o, int o_dtype,
                                                     const float* k_scale_pool, const void* km, float* lse, int B, int Hq,
                                                     int Hk, int M, int D, int qk_gran, int warpq, float sm_scale,
                                                     const int32_t* block_table, int64_t table_stride, int max_pages,
                                                     int page_size, int num_pages, const int32_t* kv_lens, int num_splits,
                                                     int causal, int q_fold, void* workspace, size_t workspace_bytes,
                                                     sage_stream_t stream) {
  return splitkv_paged_entry(q, q_dtype, k8_pool, v_pool, v_dtype, o, o_dtype, k_scale_pool, km, false, nullptr, lse, B, Hq, Hk,
                             M, D, qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages,
                             kv_lens, num_splits, causal, q_fold, workspace, workspace_bytes, stream);
}

extern "C" int sage_attn_fusedq_pv_f8_splitkv_paged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                    const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
                                                    const float* k_scale_pool, const void* km, const float* v_scale, float* lse,
                                                    int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq, float sm_scale,
                                                    const int32_t* block_table, int64_t table_stride, int max_pages,
                                                    int page_size, int num_pages, const int32_t* kv_lens, int num_splits,
                                                    int causal, int q_fold, void* workspace, size_t workspace_bytes,
                                                    sage_stream_t stream) {
  return splitkv_paged_entry(q, q_dtype, k8_pool, v8_pool, SAGE_F16, o, o_dtype, k_scale_pool, km, true, v_scale, lse, B, Hq,
                             Hk, M, D, qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages,
                             kv_lens, num_splits, causal, q_fold, workspace, workspace_bytes, stream);
}
