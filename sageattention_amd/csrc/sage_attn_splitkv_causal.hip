// Causal split-KV attention (the rule: include/sageattn_hip.h, sage_attn_fusedq_pv_*_splitkv_causal): attn_i8_splitkv_kernel
// (sage_attn_splitkv.hip) with a diagonal that is aligned to the END of the batch's keys.  The M query rows are T = M / g
// tokens of g folded query heads each (g = q_fold; row r is token r / g), and the tokens are the last T positions of the
// batch's len_b valid keys: token t attends the keys 0 .. t + off_b, off_b = len_b - T, which moves with kv_lens[b] on the
// device.  The body is sage_attn_body.h with CAUSAL = true, SPLITKV = true: the split's range and the moved operands of the
// non-causal form, and the causal machinery of the dense kernel (wave_tiles, n_plain, mask_limit) on a per-lane limit
// `token + off_b - 64 * (first tile of the split)` in place of the row index.
//
// A row whose keys in a split are all masked: every score of it is the -inf pattern, so its row maxima are -inf, no rescale
// ever fires for it and m_run keeps its start -1e30; every p is exp2(-inf) = 0, so l_run = 0 (on the matrix pipe as well:
// a sum of zeros), inv = 1 / 0 = inf, the fp32 partial row is 0 * inf = NaN and the partial lse2 is -1e30 + log2(0) = -inf.
// The merge drops exactly such a slot by select (`l != -inf`) and never multiplies it: no per-row branch in the loop.  A row
// that keeps a key only in a LATER tile of the split starts the same way and is rescaled by alpha = exp2(-1e30 - m) = 0.
//
// A kernel of its own name and a source file of its own, as every other twin: the build's guards match kernels by name, and
// the other instantiations keep their code and their registers.
#include "sage_attn_launch.h"

namespace sage {

template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
// (register budget as attn_i8_kernel: head_dim 64 FP8 PV with 4 waves is held to three waves per SIMD)
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_splitkv_causal_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = true, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// The merge: splitkv_merge_kernel (sage_attn_splitkv.hip) with the count of splits of the row's Q-BLOCK.  Workgroup
// (b, h, qb, s) of the kernel above ran iff 64 * s * tps_b < end_qb, the key bound of the q-block's last row < M; the same
// count is derived here, min(count_b, ceil(ceil(end_qb / 64) / tps_b)), and no slot at or beyond it is loaded.  Inside the
// count every row < M of the q-block was written by every split: a row without a key there holds NaN / -inf and is dropped by
// the select; a row without a key anywhere ends as o = 0, lse = -inf (sum = 0).  A q-block with count 0 -- a chunk longer
// than the batch's keys, or a batch without keys -- gets o = 0, lse = -inf and reads neither the workspace nor the parked
// correction, which no workgroup wrote.  MAXC: compile-time bound of S (2, 4, 8 or 16).
template <bool BF16, int MAXC>
__global__ __launch_bounds__(256) void splitkv_causal_merge_kernel(const AttnParams p, const int D) {
  const int tpr = D / 4;
  const int64_t rows = (int64_t)p.B * p.Hq * p.M;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = gid / tpr;
  const int c = (int)(gid % tpr);
  if (row >= rows) return;
  const int m = (int)(row % p.M);
  const int64_t bh = row / p.M;
  const int h = (int)(bh % p.Hq), b = (int)(bh / p.Hq);
  int len_b = p.N;
  if (p.kv_lens) len_b = min(max(p.kv_lens[b], 0), p.N);
  const int ntk_b = (len_b + 63) >> 6, tps_b = (ntk_b + p.num_splits - 1) / p.num_splits;
  // key bound of the last row < M of the row's q-block: (its token - T) + len_b + 1, in this order (no overflow)
  const int tok = min((m | 127), p.M - 1) / p.q_fold;
  const int end_qb = min(len_b, (tok - p.M / p.q_fold) + len_b + 1);
  const int count = end_qb > 0 ? min((ntk_b + tps_b - 1) / tps_b, (((end_qb + 63) >> 6) + tps_b - 1) / tps_b) : 0;
  uint16_t* const op = p.o + b * p.osb + h * p.osh + (int64_t)m * p.osn + c * 4;
  if (count == 0) {
    *reinterpret_cast<uint2*>(op) = make_uint2(0u, 0u);
    if (c == 0 && p.lse) p.lse[row] = -INFINITY;
    return;
  }
  float l[MAXC];
  float4 raw[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int s = i < count ? i : count - 1;
    l[i] = p.sk_lse[(int64_t)s * rows + row];
    raw[i] = *reinterpret_cast<const float4*>(p.sk_o + ((int64_t)s * rows + row) * D + c * 4);
  }
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) mx = i < count ? fmaxf(mx, l[i]) : mx;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {  // split order: deterministic
    const bool use = i < count && l[i] != -INFINITY;
    const float w = exp2f(l[i] - mx);
    sum = use ? sum + w : sum;
    const float f[4] = {raw[i].x, raw[i].y, raw[i].z, raw[i].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = use ? acc[j] + f[j] * w : acc[j];
  }
  const float inv = sum > 0.f ? 1.0f / sum : 0.f;
  uint2 w2;
  w2.x = (uint32_t)f32_to_elem_bits<BF16>(acc[0] * inv) | ((uint32_t)f32_to_elem_bits<BF16>(acc[1] * inv) << 16);
  w2.y = (uint32_t)f32_to_elem_bits<BF16>(acc[2] * inv) | ((uint32_t)f32_to_elem_bits<BF16>(acc[3] * inv) << 16);
  *reinterpret_cast<uint2*>(op) = w2;
  if (c == 0 && p.lse) {
    // as splitkv_merge_kernel: natural log, then the correction q . km that split 0 parked in the slot (count > 0: it ran).
    // A row without a key has sum = 0: -inf, whatever the finite correction is
#pragma clang fp contract(off)
    float v = (sum > 0.f ? mx + log2f(sum) : -INFINITY) / 1.44269504f;
    v += p.lse[row] * p.sm_scale;
    p.lse[row] = v;
  }
}

// the attention launch over (b, h, q-block, split), then the merge: launch_splitkv goes through it for c.splitkv_causal
int launch_splitkv_causal(const AttnCall& c, hipStream_t st) {
  const AttnParams& p = c.p;
  const int s = by_dim(c.D, [&](auto d) {
    return by_flag(c.pv_fp8, [&](auto fp8) {
      constexpr int D = decltype(d)::value;
      constexpr bool PV_FP8 = decltype(fp8)::value;
      constexpr size_t smem = attn_lds_bytes(D, 4, PV_FP8);
      return by_flag(c.kthread, [&](auto k) {
        return by_flag(!PV_FP8 && c.v_bf16, [&](auto v) {  // fp8 V has no bf16 flavour
          auto kern = attn_i8_splitkv_causal_kernel<D, decltype(k)::value, !PV_FP8 && decltype(v)::value, PV_FP8>;
          if (!allow_lds((const void*)kern, smem)) return (int)SAGE_ERR_LAUNCH;
          hipLaunchKernelGGL(kern, dim3(p.nqb * p.Hq * p.B * p.num_splits), dim3(256), smem, st, p);
          return launch_status();
        });
      });
    });
  });
  if (s) return s;
  const int64_t threads = (int64_t)p.B * p.Hq * p.M * (c.D / 4);
  by_flag(p.out_bf16 != 0, [&](auto bf) {
    by_slots(p.num_splits, [&](auto slots) {
      hipLaunchKernelGGL((splitkv_causal_merge_kernel<decltype(bf)::value, decltype(slots)::value>),
                         dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, p, c.D);
    });
  });
  return launch_status();
}

}  // namespace sage

using namespace sage;

extern "C" int sage_attn_fusedq_pv_f16_splitkv_causal(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                      const sage_tensor* v, int v_dtype, const sage_tensor* o, int o_dtype,
                                                      const float* k_scale, const void* km, const float* v_mean, float* lse,
                                                      int B, int Hq, int Hk, int M, int N, int D, int qk_gran, int warpq,
                                                      float sm_scale, const int32_t* kv_lens, int num_splits, int q_fold,
                                                      void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  AttnArgs a = splitkv_args(q, q_dtype, k8, v, v_dtype, o, o_dtype, k_scale, km, nullptr, v_mean, lse, B, Hq, Hk, M, N, D,
                            qk_gran, warpq, sm_scale, kv_lens, num_splits, workspace, workspace_bytes);
  a.split_causal = true; a.q_fold = q_fold;
  return run_splitkv(a, q_dtype, stream);
}

extern "C" int sage_attn_fusedq_pv_f8_splitkv_causal(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                     const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                                     const float* k_scale, const void* km, const float* v_scale,
                                                     const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N,
                                                     int D, int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens,
                                                     int num_splits, int q_fold, void* workspace, size_t workspace_bytes,
                                                     sage_stream_t stream) {
  if (!v_scale) return SAGE_ERR_INVALID_ARGUMENT;
  AttnArgs a = splitkv_args(q, q_dtype, k8, v_fp8, SAGE_F16, o, o_dtype, k_scale, km, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                            qk_gran, warpq, sm_scale, kv_lens, num_splits, workspace, workspace_bytes);
  a.split_causal = true; a.q_fold = q_fold;
  return run_splitkv(a, q_dtype, stream);
}
