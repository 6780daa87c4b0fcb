// Split-KV attention (the rule: include/sageattn_hip.h, sage_attn_fusedq_pv_*_splitkv): the loop body of sage_attn.hip with
// SPLITKV = true, then the merge of the partial results.  The other attention kernels launch one workgroup per (b, h_q, 128-row
// q-block), which walks every key tile of its head: few query rows against many keys leave most of the chip idle.  Here the
// grid has a fourth factor, S = num_splits: workgroup (b, h, q-block, s) is the dense 4-wave kernel on the key tiles
// [s * tps_b, min((s + 1) * tps_b, ntk_b)) of its batch -- the same pipelined loop, fused Q quantizer, per-thread and per-warp
// scales, FP16 / BF16 / FP8 P.V, GQA, both head dims, an optional per-batch key length -- and stores its normalised fp32
// output rows and raw base-2 LSEs into the caller's workspace.  splitkv_merge_kernel then combines the non-empty splits of
// every row in split order (no atomics: deterministic), rounds once to the output type and finishes the LSE.
//
// A kernel of its own name and a source file of its own, as attn_i8_kvlen_kernel: the build's occupancy guard matches kernels
// by name, and the other instantiations keep their code and their registers.  The causal attention kernel is the twin of
// sage_attn_splitkv_causal.hip; what the two forms share is here once: the merge kernel (a template flag CAUSAL), its launch
// and the four entry points.  attn_launch (sage_attn.hip) runs the attention kernel of the call's form, then the merge.
#include "sage_attn_launch.h"

namespace sage {

template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
// (register budget as attn_i8_kernel: head_dim 64 FP8 PV with 4 waves is held to three waves per SIMD)
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_splitkv_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = false, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true, PAGED = false;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// The merge.  One thread per 4 output channels of a row (b, h, m); the arithmetic is merge_many_kernel's (sage_misc.hip) on
// base-2 LSEs: mx = max_s l_s, w_s = exp2(l_s - mx), o = sum_s w_s o_s / sum_s w_s, lse2 = mx + log2(sum_s w_s), in split
// order.  `count`, the number of slots the row merges, is derived here, from kv_lens (or N) and S, exactly as the attention
// workgroups derive their ranges: slots at or beyond it were not written by this call and may hold anything, NaN included --
// they are not loaded (a slot index past the count repeats the last valid one) and their terms are dropped by selects, never
// multiplied by zero.  Every lse and every o run of the thread is requested up front, slots unrolled, for the reason given
// in merge_many_kernel: under a branch per slot each split costs two dependent round trips.
// CAUSAL: the merge of attn_i8_splitkv_causal_kernel (sage_attn_splitkv_causal.hip), else of the kernel above; the
// non-causal form does not read p.q_fold.  MAXC: compile-time bound of S (2, 4, 8 or 16).
template <bool BF16, int MAXC, bool CAUSAL>
__global__ __launch_bounds__(256) void splitkv_merge_kernel(const AttnParams p, const int D) {
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
  int count;
  if constexpr (CAUSAL) {
    // The count of splits of the row's Q-BLOCK.  Workgroup (b, h, qb, s) of the causal kernel ran iff 64 * s * tps_b < end_qb,
    // the key bound of the q-block's last row < M; the same count is derived here, min(count_b, ceil(ceil(end_qb / 64) /
    // tps_b)).  Inside the count every row < M of the q-block was written by every split: a row without a key there holds
    // NaN / -inf and is dropped by the select; a row without a key anywhere ends as o = 0, lse = -inf (sum = 0).  A q-block
    // with count 0 is a chunk longer than the batch's keys, or a batch without keys.
    // end_qb: (the last row's token - T) + len_b + 1, in this order (no overflow)
    const int tok = min((m | 127), p.M - 1) / p.q_fold;
    const int end_qb = min(len_b, (tok - p.M / p.q_fold) + len_b + 1);
    count = end_qb > 0 ? min((ntk_b + tps_b - 1) / tps_b, (((end_qb + 63) >> 6) + tps_b - 1) / tps_b) : 0;
  } else {
    count = tps_b > 0 ? (ntk_b + tps_b - 1) / tps_b : 0;  // the non-empty splits of the row's batch
  }
  uint16_t* const op = p.o + b * p.osb + h * p.osh + (int64_t)m * p.osn + c * 4;
  if (count == 0) {  // no split ran: o = 0, lse = -inf; nothing of the workspace (or of the parked correction) is read
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
    // natural log of the merged base-2 LSE, then the smoothing correction q . km that split 0 parked in the slot (count > 0:
    // it ran): product and sum rounded separately, as the fused-Q epilogue of the attention kernels and sage_finish_lse do.
    // A row without a key has sum = 0: -inf, whatever the finite correction is
#pragma clang fp contract(off)
    float v = (sum > 0.f ? mx + log2f(sum) : -INFINITY) / 1.44269504f;
    v += p.lse[row] * p.sm_scale;
    p.lse[row] = v;
  }
}

// the attention launch over (b, h, q-block, split) of a non-causal call
int launch_splitkv_attn(const AttnCall& c, hipStream_t st) {
  return launch_4wave_kernel(c, st, c.p.nqb * c.p.Hq * c.p.B * c.p.num_splits, [](auto d, auto k, auto v, auto fp8) {
    return attn_i8_splitkv_kernel<decltype(d)::value, decltype(k)::value, decltype(v)::value, decltype(fp8)::value>;
  });
}

// the merge of a split-KV call, causal (c.splitkv_causal) or not
int launch_splitkv_merge(const AttnCall& c, hipStream_t st) {
  const AttnParams& p = c.p;
  const int64_t threads = (int64_t)p.B * p.Hq * p.M * (c.D / 4);
  by_flag(p.out_bf16 != 0, [&](auto bf) {
    by_flag(c.splitkv_causal, [&](auto causal) {
      by_slots(p.num_splits, [&](auto slots) {
        hipLaunchKernelGGL((splitkv_merge_kernel<decltype(bf)::value, decltype(slots)::value, decltype(causal)::value>),
                           dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, p, c.D);
      });
    });
  });
  return launch_status();
}

// A split-KV entry point (there is no INT8-Q form): the fused-Q argument block -- 128-row q-blocks, the kernel applies
// sm_scale -- then check and launch.  pv_fp8: the f8 forms, which need v_scale (null in the FP16 / BF16 forms); causal: the
// *_splitkv_causal forms with their q_fold.
static int splitkv_entry(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                         const sage_tensor* o, int o_dtype, const float* k_scale, const void* km, bool pv_fp8,
                         const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                         int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens, int num_splits, bool causal,
                         int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  if (pv_fp8 && !v_scale) return SAGE_ERR_INVALID_ARGUMENT;
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  AttnArgs a;
  a.q = q; a.q_dtype = q_dtype; a.k8 = k8; a.v = v; a.v_dtype = v_dtype; a.o = o; a.o_dtype = o_dtype; a.k_scale = k_scale;
  a.km = km; a.v_scale = v_scale; a.pv_fp8 = pv_fp8; a.v_mean = v_mean; a.lse = lse;
  a.B = B; a.Hq = Hq; a.Hk = Hk; a.M = M; a.N = N; a.D = D; a.qk_gran = qk_gran; a.blkq = 128; a.warpq = warpq;
  a.sm_scale = sm_scale;
  a.split_kv = true; a.split_kv_lens = kv_lens; a.num_splits = num_splits; a.split_workspace = workspace;
  a.split_workspace_bytes = workspace_bytes;
  a.split_causal = causal; a.q_fold = q_fold;
  AttnCall c;
  if (const int s = attn_check(c, a)) return s;
  return attn_launch(c, (hipStream_t)stream);
}

}  // namespace sage

using namespace sage;

extern "C" size_t sage_splitkv_workspace_bytes(int B, int Hq, int M, int D, int num_splits) {
  if (B <= 0 || Hq <= 0 || M <= 0 || D <= 0 || num_splits < 1 || num_splits > SAGE_MERGE_MAX) return 0;
  return (size_t)splitkv_bytes(B, Hq, M, D, num_splits);
}

extern "C" int sage_attn_fusedq_pv_f16_splitkv(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v,
                                               int v_dtype, const sage_tensor* o, int o_dtype, const float* k_scale,
                                               const void* km, const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                               int N, int D, int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens,
                                               int num_splits, void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  return splitkv_entry(q, q_dtype, k8, v, v_dtype, o, o_dtype, k_scale, km, false, nullptr, v_mean, lse, B, Hq, Hk, M, N, D,
                       qk_gran, warpq, sm_scale, kv_lens, num_splits, false, 1, workspace, workspace_bytes, stream);
}

extern "C" int sage_attn_fusedq_pv_f8_splitkv(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_fp8,
                                              const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                              const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk,
                                              int M, int N, int D, int qk_gran, int warpq, float sm_scale,
                                              const int32_t* kv_lens, int num_splits, void* workspace, size_t workspace_bytes,
                                              sage_stream_t stream) {
  return splitkv_entry(q, q_dtype, k8, v_fp8, SAGE_F16, o, o_dtype, k_scale, km, true, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                       qk_gran, warpq, sm_scale, kv_lens, num_splits, false, 1, workspace, workspace_bytes, stream);
}

extern "C" int sage_attn_fusedq_pv_f16_splitkv_causal(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                      const sage_tensor* v, int v_dtype, const sage_tensor* o, int o_dtype,
                                                      const float* k_scale, const void* km, const float* v_mean, float* lse,
                                                      int B, int Hq, int Hk, int M, int N, int D, int qk_gran, int warpq,
                                                      float sm_scale, const int32_t* kv_lens, int num_splits, int q_fold,
                                                      void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  return splitkv_entry(q, q_dtype, k8, v, v_dtype, o, o_dtype, k_scale, km, false, nullptr, v_mean, lse, B, Hq, Hk, M, N, D,
                       qk_gran, warpq, sm_scale, kv_lens, num_splits, true, q_fold, workspace, workspace_bytes, stream);
}

extern "C" int sage_attn_fusedq_pv_f8_splitkv_causal(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                     const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                                     const float* k_scale, const void* km, const float* v_scale,
                                                     const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N,
                                                     int D, int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens,
                                                     int num_splits, int q_fold, void* workspace, size_t workspace_bytes,
                                                     sage_stream_t stream) {
  return splitkv_entry(q, q_dtype, k8, v_fp8, SAGE_F16, o, o_dtype, k_scale, km, true, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                       qk_gran, warpq, sm_scale, kv_lens, num_splits, true, q_fold, workspace, workspace_bytes, stream);
}
