// Sliding-window attention and sink logits on the paged KV cache (the rule: include/sageattn_hip_window.h).  Four kernels:
//
//  * attn_i8_splitkv_causal_paged_window_kernel: sage_attn_body.h with CAUSAL, SPLITKV, PAGED and the macro
//    SAGE_ATTN_BODY_WINDOW.  A workgroup is (b, h, q-block, split) as in the causal paged kernel, but the q-block's tile range
//    starts at the tile of its first row's lower limit, tlo, and the splits cut [tlo, thi]: sk_t0 = tlo + split * tps moves the
//    page lookups, the K scales and the descriptors, so tiles and table entries below the window are never named.  The lower
//    limit of a lane has no register of its own: mask_limit forms it from the upper one, lim_l - window + 1, in a second pass
//    of the select and only where the tile needs it.  The wave's left-masked tiles -- a wave spans at most 32 tokens, the
//    q-block 128 -- run as run-time-slot iterations in front of the fast loop (the hand-placed stream; at FP8 PV and head_dim
//    128 the compiler-scheduled body): a multiple of the ring, so that the fast loop keeps its compile-time slots, or all of
//    the wave's tiles but the last where it has no more than that.
//  * attn_i8_splitkv_causal_paged_ragged_window_kernel: the same with SAGE_ATTN_BODY_RAGGED, on the work list of
//    sage_ragged_q_plan.
//  * window_merge_kernel / ragged_window_merge_kernel: the arithmetic of splitkv_merge_kernel / ragged_merge_kernel in split
//    order, with the split count of the q-block's window range, then the sink term: lse' = logaddexp(lse, sink_h) on the corrected
//    natural-log LSE, o' = o * exp(lse - lse'), one rounding to the output type.
//
// window and sinks travel beside the parameter block (WindowParams), so AttnParams and every other kernel keep their layout
// and their code.  A source file and kernel names of their own, as every other twin: the build's guards match kernels by name.
#include <climits>
#include "../../include/sageattn_hip_window.h"
#include "sage_attn_launch.h"

namespace sage {

struct WindowParams {
  AttnParams a;
  const float* sinks;  // fp32 [query heads of the un-folded view] or null
  int window;          // 1 .. a.N
};

// ---- the attention kernels ---------------------------------------------------------------------------------------------------
template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
// (register budget as attn_i8_kernel: head_dim 64 FP8 PV with 4 waves is held to three waves per SIMD)
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_splitkv_causal_paged_window_kernel(const WindowParams wp) {
  const AttnParams& p = wp.a;
  const int sw_window = wp.window;
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = true, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true, PAGED = true;
#define SAGE_ATTN_BODY_OF_KERNEL
#define SAGE_ATTN_BODY_WINDOW
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_WINDOW
#undef SAGE_ATTN_BODY_OF_KERNEL
}

template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_splitkv_causal_paged_ragged_window_kernel(const WindowParams wp) {
  const AttnParams& p = wp.a;
  const int sw_window = wp.window;
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = true, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true, PAGED = true;
#define SAGE_ATTN_BODY_OF_KERNEL
#define SAGE_ATTN_BODY_RAGGED
#define SAGE_ATTN_BODY_WINDOW
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_WINDOW
#undef SAGE_ATTN_BODY_RAGGED
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// ---- the merge -----------------------------------------------------------------------------------------------------------------
// One thread per 4 output channels of a row.  m is the row within its sequence of M = T_b * g rows and len_b keys, `row` its
// slot in a split's partials and `rows` the slots of one split; op / lp are the row's output run and LSE slot (lp null: no LSE,
// and then no sinks), head its un-folded query head.  count is the number of splits that ran for the row's q-block, from the
// range rule exactly as the attention workgroups derive it; slots at or beyond it are not loaded.  mx, sum, acc and the LSE tail
// are those of splitkv_merge_kernel, the same operations in the same order: without sinks the row has that merge's bits.
// The parked correction is read by every thread of the row (they share a wave, and the one store to the slot depends on that
// load), because with sinks every thread needs the corrected LSE.
template <bool BF16, int MAXC>
__device__ __forceinline__ void window_merge_row(const AttnParams& p, const int D, const int window, const float* sinks,
                                                 const int c, const int m, const int M, const int len_b, const int64_t row,
                                                 const int64_t rows, uint16_t* const op, float* const lp, const int head) {
  const int g = p.q_fold;
  const int off = len_b - M / g;
  const int lo = max((m & ~127) / g + off - window + 1, 0);
  const int hi = min(min(m | 127, M - 1) / g + off, len_b - 1);
  int count = 0;
  if (hi >= 0) {
    const int nt = (hi >> 6) - (lo >> 6) + 1, tps = (nt + p.num_splits - 1) / p.num_splits;
    count = (nt + tps - 1) / tps;
  }
  if (count == 0) {  // no split ran: o = 0, lse = -inf; nothing of the workspace (or of the parked correction) is read
    *reinterpret_cast<uint2*>(op) = make_uint2(0u, 0u);
    if (c == 0 && lp) *lp = -INFINITY;
    return;
  }
  float l[MAXC];
  float4 raw[MAXC];
#pragma unroll
  for (int k = 0; k < MAXC; ++k) {
    const int s = k < count ? k : count - 1;
    l[k] = p.sk_lse[(int64_t)s * rows + row];
    raw[k] = *reinterpret_cast<const float4*>(p.sk_o + ((int64_t)s * rows + row) * D + c * 4);
  }
  const float corr = lp ? *lp : 0.f;
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < MAXC; ++k) mx = k < count ? fmaxf(mx, l[k]) : mx;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < MAXC; ++k) {  // split order: deterministic
    const bool use = k < count && l[k] != -INFINITY;
    const float w = exp2f(l[k] - mx);
    sum = use ? sum + w : sum;
    const float f[4] = {raw[k].x, raw[k].y, raw[k].z, raw[k].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = use ? acc[j] + f[j] * w : acc[j];
  }
  const float inv = sum > 0.f ? 1.0f / sum : 0.f;
  // natural log of the merged base-2 LSE, then the correction q . km that split 0 parked in the slot; product and sum rounded
  // separately, as in splitkv_merge_kernel
  float v, keep = 1.0f;
  {
#pragma clang fp contract(off)
    v = (sum > 0.f ? mx + log2f(sum) : -INFINITY) / 1.44269504f;
    v += corr * p.sm_scale;
    if (sinks && sum > 0.f) {  // (a row without a key stays o = 0, lse = -inf)
      const float sk = sinks[head];
      const float top = fmaxf(v, sk);
      const float v2 = top + logf(expf(v - top) + expf(sk - top));
      keep = expf(v - v2);
      v = v2;
    }
  }
  // (without sinks the statement of splitkv_merge_kernel, word for word: hipcc folds its multiply and convert into one
  //  instruction with one rounding, and a select in between would cost the bit anchor an ulp here and there)
  uint2 w2;
  if (sinks) {
    const float k2 = inv * keep;
    w2.x = (uint32_t)f32_to_elem_bits<BF16>(acc[0] * k2) | ((uint32_t)f32_to_elem_bits<BF16>(acc[1] * k2) << 16);
    w2.y = (uint32_t)f32_to_elem_bits<BF16>(acc[2] * k2) | ((uint32_t)f32_to_elem_bits<BF16>(acc[3] * k2) << 16);
  } else {
    w2.x = (uint32_t)f32_to_elem_bits<BF16>(acc[0] * inv) | ((uint32_t)f32_to_elem_bits<BF16>(acc[1] * inv) << 16);
    w2.y = (uint32_t)f32_to_elem_bits<BF16>(acc[2] * inv) | ((uint32_t)f32_to_elem_bits<BF16>(acc[3] * inv) << 16);
  }
  *reinterpret_cast<uint2*>(op) = w2;
  if (c == 0 && lp) *lp = v;
}

// the rows of a [B, Hq, M] call, as splitkv_merge_kernel walks them
template <bool BF16, int MAXC>
__global__ __launch_bounds__(256) void window_merge_kernel(const WindowParams wp, const int D) {
  const AttnParams& p = wp.a;
  const int tpr = D / 4;
  const int64_t rows = (int64_t)p.B * p.Hq * p.M;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = gid / tpr;
  const int c = (int)(gid % tpr);
  if (row >= rows) return;
  const int m = (int)(row % p.M);
  const int64_t bh = row / p.M;
  const int h = (int)(bh % p.Hq), b = (int)(bh / p.Hq);
  const int len_b = min(max(p.kv_lens[b], 0), p.N);
  window_merge_row<BF16, MAXC>(p, D, wp.window, wp.sinks, c, m, p.M, len_b, row, rows,
                               p.o + b * p.osb + h * p.osh + (int64_t)m * p.osn + c * 4, p.lse ? p.lse + row : nullptr,
                               h * p.q_fold + m % p.q_fold);
}

// the rows of the work list, as ragged_merge_kernel walks them: one workgroup per (work item, head, run of 256 / (D / 4) rows)
template <bool BF16, int MAXC>
__global__ __launch_bounds__(256) void ragged_window_merge_kernel(const WindowParams wp, const int D) {
  const AttnParams& p = wp.a;
  const int tpr = D / 4, rpb = 256 / tpr, runs = 128 / rpb;
  const int run = blockIdx.x % runs;
  const int ih = blockIdx.x / runs;
  const int h = ih / p.nqb;
  const int2 item = *reinterpret_cast<const int2*>(p.rq_items + 2 * (ih % p.nqb));
  const int b = item.x, qb = item.y;
  if (b < 0) return;
  const int g = p.q_fold;
  const int total = p.M / g;
  const int q_lo = min(max(p.cu_q[b], 0), total);
  const int T = min(max(p.cu_q[b + 1] - q_lo, 0), total - q_lo);
  const int M = T * g;
  const int m = qb * 128 + run * rpb + (int)threadIdx.x / tpr;
  const int c = (int)threadIdx.x % tpr;
  if (m >= M) return;
  const int len_b = min(max(p.kv_lens[b], 0), p.N);
  const int t = m / g, i = m - t * g;
  const int64_t token = q_lo + t;
  const int head = h * g + i;
  window_merge_row<BF16, MAXC>(p, D, wp.window, wp.sinks, c, m, M, len_b, (int64_t)h * p.M + (int64_t)q_lo * g + m,
                               (int64_t)p.Hq * p.M, p.o + token * p.osn + head * p.osh + c * 4,
                               p.lse ? p.lse + token * ((int64_t)p.Hq * g) + head : nullptr, head);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// launch_4wave_kernel (sage_attn_launch.h) for kernels that take WindowParams
template <class KernelOf>
static int launch_window_kernel(const AttnCall& c, const WindowParams& wp, hipStream_t st, int grid, KernelOf kernel_of) {
  return by_dim(c.D, [&](auto d) {
    return by_flag(c.pv_fp8, [&](auto fp8) {
      constexpr int D = decltype(d)::value;
      constexpr bool PV_FP8 = decltype(fp8)::value;
      constexpr size_t smem = attn_lds_bytes(D, 4, PV_FP8);
      return by_flag(c.kthread, [&](auto k) {
        return by_flag(c.v_bf16, [&](auto v) {
          void (*kern)(const WindowParams) = kernel_of(d, k, std::bool_constant<!PV_FP8 && decltype(v)::value>{}, fp8);
          if (!allow_lds((const void*)kern, smem)) return (int)SAGE_ERR_LAUNCH;
          hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, wp);
          return launch_status();
        });
      });
    });
  });
}

// Both forms (cu == nullptr: the [B, Hq, M, D] form, `M` its rows; else the ragged form, `M` its total_tokens).  What is the
// window's own is checked here, the rest as the parents check it; nothing is enqueued before every check has passed.
static int window_entry(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                        const sage_tensor* o, int o_dtype, const float* k_scale, const void* km, bool pv_fp8,
                        const float* v_scale, float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq,
                        float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                        int num_pages, const int32_t* kv_lens, const int32_t* cu, const int32_t* items, int n_items,
                        int num_splits, int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream, int window,
                        const float* sinks) {
  const bool ragged = cu != nullptr;
  if (window < 1 || ((uintptr_t)sinks & 3) || (sinks && !lse)) return SAGE_ERR_INVALID_ARGUMENT;
  if (pv_fp8 && !v_scale) return SAGE_ERR_INVALID_ARGUMENT;
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  if (page_size != 64 && page_size != 128 && page_size != 256) return SAGE_ERR_INVALID_ARGUMENT;
  if (!block_table || ((uintptr_t)block_table & 3) || !kv_lens || max_pages < 1 || num_pages < 1 || table_stride < max_pages ||
      table_stride > INT_MAX)
    return SAGE_ERR_INVALID_ARGUMENT;
  if ((int64_t)max_pages * page_size > INT_MAX) return SAGE_ERR_TOO_LARGE;
  int Hf = Hq;
  sage_tensor qv, ov;
  if (ragged) {
    if (B <= 0 || Hq <= 0 || Hk <= 0 || Hq % Hk != 0 || M < 1) return SAGE_ERR_INVALID_ARGUMENT;
    if (q_fold != 1 && q_fold != Hq / Hk) return SAGE_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)cu & 3) || !items || ((uintptr_t)items & 7) || !q || !o) return SAGE_ERR_INVALID_ARGUMENT;
    const int64_t rows = (int64_t)M * q_fold;
    if (rows > INT_MAX || rows / 128 + B > INT_MAX / 256) return SAGE_ERR_TOO_LARGE;
    if (n_items != rows / 128 + B) return SAGE_ERR_INVALID_ARGUMENT;
    Hf = Hq / q_fold;
    if ((int64_t)n_items * Hf * num_splits > INT_MAX || (int64_t)n_items * Hf * (D / 8) > INT_MAX) return SAGE_ERR_TOO_LARGE;
    // the folded view as ONE batch of Hq / g heads and total_tokens * g rows, as in sage_attn_splitkv_ragged.hip
    qv = {q->data, 0, q->stride_h, q->stride_n};
    ov = {o->data, 0, o->stride_h, o->stride_n};
  }
  AttnArgs a;
  a.q = ragged ? &qv : q; a.q_dtype = q_dtype; a.k8 = k8; a.v = v; a.v_dtype = v_dtype; a.o = ragged ? &ov : o; a.o_dtype = o_dtype;
  a.k_scale = k_scale; a.km = km; a.v_scale = v_scale; a.pv_fp8 = pv_fp8; a.lse = lse;
  a.B = ragged ? 1 : B; a.Hq = Hf; a.Hk = Hk; a.M = ragged ? M * q_fold : M; a.N = max_pages * page_size; a.D = D;
  a.qk_gran = qk_gran; a.blkq = 128; a.warpq = warpq; a.sm_scale = sm_scale;
  a.split_kv = true; a.split_kv_lens = kv_lens; a.num_splits = num_splits; a.split_workspace = workspace;
  a.split_workspace_bytes = workspace_bytes;
  a.split_causal = true; a.q_fold = q_fold;
  a.paged = true; a.block_table = block_table; a.table_stride = (int)table_stride; a.page_size = page_size;
  AttnCall c;
  if (const int s = attn_check(c, a)) return s;
  WindowParams wp;
  wp.a = c.p;
  wp.sinks = sinks;
  wp.window = window < a.N ? window : a.N;  // (a window beyond the capacity is the capacity: the limits below then cannot overflow)
  hipStream_t st = (hipStream_t)stream;
  if (ragged) {  // (the words of cu_q, v_mean and nqb; B counts the sequences again)
    wp.a.B = B; wp.a.cu_q = cu; wp.a.rq_items = items; wp.a.nqb = n_items;
    const int s = launch_window_kernel(c, wp, st, n_items * Hf * num_splits, [](auto d, auto k, auto vb, auto fp8) {
      return attn_i8_splitkv_causal_paged_ragged_window_kernel<decltype(d)::value, decltype(k)::value, decltype(vb)::value,
                                                               decltype(fp8)::value>;
    });
    if (s) return s;
    by_flag(c.p.out_bf16 != 0, [&](auto bf) {
      by_slots(num_splits, [&](auto slots) {
        hipLaunchKernelGGL((ragged_window_merge_kernel<decltype(bf)::value, decltype(slots)::value>),
                           dim3((unsigned)(n_items * Hf * (D / 8))), dim3(256), 0, st, wp, D);
      });
    });
    return launch_status();
  }
  if ((int64_t)c.p.nqb * Hq * B * num_splits > INT_MAX) return SAGE_ERR_TOO_LARGE;
  const int s = launch_window_kernel(c, wp, st, c.p.nqb * Hq * B * num_splits, [](auto d, auto k, auto vb, auto fp8) {
    return attn_i8_splitkv_causal_paged_window_kernel<decltype(d)::value, decltype(k)::value, decltype(vb)::value,
                                                      decltype(fp8)::value>;
  });
  return s ? s : launch_window_merge(c, wp.window, sinks, st);
}

// (declared in sage_attn_launch.h: sage_attn_decode_window.hip merges its splits with it as well)
int launch_window_merge(const AttnCall& c, int window, const float* sinks, hipStream_t st) {
  WindowParams wp;
  wp.a = c.p;
  wp.sinks = sinks;
  wp.window = window;
  const int64_t threads = (int64_t)c.p.B * c.p.Hq * c.p.M * (c.D / 4);
  by_flag(c.p.out_bf16 != 0, [&](auto bf) {
    by_slots(c.p.num_splits, [&](auto slots) {
      hipLaunchKernelGGL((window_merge_kernel<decltype(bf)::value, decltype(slots)::value>),
                         dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, wp, c.D);
    });
  });
  return launch_status();
}

}  // namespace sage

using namespace sage;

extern "C" int sage_attn_fusedq_pv_f16_splitkv_paged_window(
    const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool, const sage_tensor* v_pool, int v_dtype, const sage_tensor* o,
    int o_dtype, const float* k_scale_pool, const void* km, float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq,
    float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size, int num_pages,
    const int32_t* kv_lens, int num_splits, int causal, int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream,
    int window, const float* sinks) {
  if (!causal) return SAGE_ERR_UNSUPPORTED;
  return window_entry(q, q_dtype, k8_pool, v_pool, v_dtype, o, o_dtype, k_scale_pool, km, false, nullptr, lse, B, Hq, Hk, M, D,
                      qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages, kv_lens, nullptr,
                      nullptr, 0, num_splits, q_fold, workspace, workspace_bytes, stream, window, sinks);
}

extern "C" int sage_attn_fusedq_pv_f8_splitkv_paged_window(
    const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool, const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
    const float* k_scale_pool, const void* km, const float* v_scale, float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran,
    int warpq, float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size, int num_pages,
    const int32_t* kv_lens, int num_splits, int causal, int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream,
    int window, const float* sinks) {
  if (!causal) return SAGE_ERR_UNSUPPORTED;
  return window_entry(q, q_dtype, k8_pool, v8_pool, SAGE_F16, o, o_dtype, k_scale_pool, km, true, v_scale, lse, B, Hq, Hk, M, D,
                      qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages, kv_lens, nullptr,
                      nullptr, 0, num_splits, q_fold, workspace, workspace_bytes, stream, window, sinks);
}

extern "C" int sage_attn_fusedq_pv_f16_splitkv_paged_ragged_window(
    const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool, const sage_tensor* v_pool, int v_dtype, const sage_tensor* o,
    int o_dtype, const float* k_scale_pool, const void* km, float* lse, int B, int Hq, int Hk, int total_tokens, int D, int qk_gran,
    int warpq, float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size, int num_pages,
    const int32_t* kv_lens, const int32_t* cu_seqlens_q, const int32_t* items, int n_items, int num_splits, int q_fold,
    void* workspace, size_t workspace_bytes, sage_stream_t stream, int window, const float* sinks) {
  if (!cu_seqlens_q) return SAGE_ERR_INVALID_ARGUMENT;
  return window_entry(q, q_dtype, k8_pool, v_pool, v_dtype, o, o_dtype, k_scale_pool, km, false, nullptr, lse, B, Hq, Hk,
                      total_tokens, D, qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages,
                      kv_lens, cu_seqlens_q, items, n_items, num_splits, q_fold, workspace, workspace_bytes, stream, window, sinks);
}

extern "C" int sage_attn_fusedq_pv_f8_splitkv_paged_ragged_window(
    const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool, const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
    const float* k_scale_pool, const void* km, const float* v_scale, float* lse, int B, int Hq, int Hk, int total_tokens, int D,
    int qk_gran, int warpq, float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
    int num_pages, const int32_t* kv_lens, const int32_t* cu_seqlens_q, const int32_t* items, int n_items, int num_splits,
    int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream, int window, const float* sinks) {
  if (!cu_seqlens_q) return SAGE_ERR_INVALID_ARGUMENT;
  return window_entry(q, q_dtype, k8_pool, v8_pool, SAGE_F16, o, o_dtype, k_scale_pool, km, true, v_scale, lse, B, Hq, Hk,
                      total_tokens, D, qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages,
                      kv_lens, cu_seqlens_q, items, n_items, num_splits, q_fold, workspace, workspace_bytes, stream, window, sinks);
}
