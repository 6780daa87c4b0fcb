// Split-KV attention on the MXFP4 V image of the KV cache (the rule: include/sageattn_hip_fp4.h): the loop body of
// sage_attn.hip with SPLITKV = true and its third P.V mode, PV_FP4, then the merge of sage_attn_splitkv.hip unchanged.
//
// The decode shapes this serves are bound by the bytes of K and V, not by arithmetic; the mode halves the V bytes once more
// on every stage they pass: HBM, the LDS-DMA copies (half as many 16-byte chunks per tile), the LDS ring (a tile is [D][32]
// bytes) and the fragment reads (one ds_read_b128 per MFMA instead of two).  The MFMA is the FP8 mode's instruction,
// v_mfma_scale_f32_32x32x64_f8f6f4, with A = V^T in e2m1 and an e8m0 scale per lane -- the scale of the lane's 32 tokens of its
// channel -- and B = P in e4m3 as before, so P, the row sums, the lazy rescale, the masks and the LSE are the FP8 mode's
// arithmetic in the same order: the LSE is bit-identical to the FP8 form's.  The scale bytes of a tile reach a VGPR by one
// load per lane, issued a tile ahead behind the P.V MFMAs, never through LDS; the epilogue has no per-channel V scale.
//
// Kernels of their own names in a file of their own, as every other twin of the body: the other instantiations keep their
// code and their registers.  Only what is dispatched is instantiated: 4 waves, fused Q, per-thread and per-warp scales.
#include "sage_attn_launch.h"
#include "../../include/sageattn_hip_fp4.h"

namespace sage {

#define SAGE_ATTN_BODY_PV_FP4
template <int D, bool KTHREAD>
// (register budget as the FP8 mode: head_dim 64 is held to three waves per SIMD)
__global__ __launch_bounds__(256, D == 64 ? 3 : 2)
void attn_i8_splitkv_v4_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool V_BF16 = false, PV_FP8 = true;
  constexpr bool CAUSAL = false, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true, PAGED = false;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

template <int D, bool KTHREAD>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2)
void attn_i8_splitkv_causal_v4_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool V_BF16 = false, PV_FP8 = true;
  constexpr bool CAUSAL = true, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true, PAGED = false;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}
#undef SAGE_ATTN_BODY_PV_FP4

// LDS of a launch: the four-slot ring of the FP8 mode with V tiles of half the size
constexpr size_t attn_v4_lds_bytes(int D) { return (size_t)attn_ring_slots(D, 4, true) * (64 * D + 32 * D); }

// An entry point: the argument block and the checks of the FP8 split-KV forms -- the image is a V^T tensor with rows of 32
// bytes per tile, the scale bytes travel in the word of v_scale -- then the attention launch and the merge.  The FP8 window
// check counts 64 bytes per tile where the image has 32: a slice it refuses is at most twice the size of one that fits.
static int splitkv_v4_entry(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_img, const sage_tensor* o,
                            int o_dtype, const float* k_scale, const void* km, const uint8_t* v_img_scale, float* lse, int B,
                            int Hq, int Hk, int M, int N, int D, int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens,
                            int num_splits, bool causal, int q_fold, void* workspace, size_t workspace_bytes,
                            sage_stream_t stream) {
  if (!v_img_scale) return SAGE_ERR_INVALID_ARGUMENT;
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  AttnArgs a;
  a.q = q; a.q_dtype = q_dtype; a.k8 = k8; a.v = v_img; a.v_dtype = SAGE_F16; a.o = o; a.o_dtype = o_dtype; a.k_scale = k_scale;
  a.km = km; a.v_scale = reinterpret_cast<const float*>(v_img_scale); a.pv_fp8 = true; a.lse = lse;
  a.B = B; a.Hq = Hq; a.Hk = Hk; a.M = M; a.N = N; a.D = D; a.qk_gran = qk_gran; a.blkq = 128; a.warpq = warpq;
  a.sm_scale = sm_scale;
  a.split_kv = true; a.split_kv_lens = kv_lens; a.num_splits = num_splits; a.split_workspace = workspace;
  a.split_workspace_bytes = workspace_bytes;
  a.split_causal = causal; a.q_fold = q_fold;
  AttnCall c;
  if (const int s = attn_check(c, a)) return s;
  c.p.v_tile_bytes = 32;  // a tile of the image is 32 bytes of every channel row
  const int grid = c.p.nqb * c.p.Hq * c.p.B * c.p.num_splits;
  const hipStream_t st = (hipStream_t)stream;
  const int s = by_dim(c.D, [&](auto d) {
    return by_flag(c.kthread, [&](auto k) {
      constexpr int DD = decltype(d)::value;
      constexpr bool KT = decltype(k)::value;
      constexpr size_t smem = attn_v4_lds_bytes(DD);
      void (*kern)(const AttnParams) = causal ? attn_i8_splitkv_causal_v4_kernel<DD, KT> : attn_i8_splitkv_v4_kernel<DD, KT>;
      if (!allow_lds((const void*)kern, smem)) return (int)SAGE_ERR_LAUNCH;
      hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, c.p);
      return launch_status();
    });
  });
  return s ? s : launch_splitkv_merge(c, st);
}

}  // namespace sage

using namespace sage;

extern "C" int sage_attn_fusedq_pv_f4_splitkv(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_img,
                                              const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                              const uint8_t* v_img_scale, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                              int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens, int num_splits,
                                              void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  return splitkv_v4_entry(q, q_dtype, k8, v_img, o, o_dtype, k_scale, km, v_img_scale, lse, B, Hq, Hk, M, N, D, qk_gran, warpq,
                          sm_scale, kv_lens, num_splits, false, 1, workspace, workspace_bytes, stream);
}

extern "C" int sage_attn_fusedq_pv_f4_splitkv_causal(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                     const sage_tensor* v_img, const sage_tensor* o, int o_dtype,
                                                     const float* k_scale, const void* km, const uint8_t* v_img_scale,
                                                     float* lse, int B, int Hq, int Hk, int M, int N, int D, int qk_gran,
                                                     int warpq, float sm_scale, const int32_t* kv_lens, int num_splits,
                                                     int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  return splitkv_v4_entry(q, q_dtype, k8, v_img, o, o_dtype, k_scale, km, v_img_scale, lse, B, Hq, Hk, M, N, D, qk_gran, warpq,
                          sm_scale, kv_lens, num_splits, true, q_fold, workspace, workspace_bytes, stream);
}
