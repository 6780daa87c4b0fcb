// Decode attention with a sliding window and sink logits on the paged KV cache, one wave per split -- and with one split ONE
// launch (the rule: include/sageattn_hip_decode_window.h).
//
// attn_i8_decode_paged_window_kernel is the text of the decode kernels, sage_attn_decode_body.h (sage_attn_decode.hip says what
// it does: a workgroup is one wave and one split of one (sequence, head), a private two-slot K / V ring in LDS filled by
// LDS-DMA and ordered by counted vmcnt waits alone, no barrier), with the statements under SAGE_ATTN_DECODE_BODY_WINDOW:
//
//  * The range.  The call is one q-block, so its keys lie between the lower limit of row 0 and the upper limit of the last row
//    < M: the tiles [tlo, thi], which the splits cut.  sk_t0 = tlo + split * tps moves the page lookups, the K scales, the
//    descriptors and the diagonal; tiles and table entries below the window are never named.
//  * The mask.  A lane's lower limit is lim_l - window + 1, formed where a tile needs it: the first dw_nlm tiles of the first
//    split that runs -- one or two, a wave spans at most 32 tokens -- take a second pass of the select, every other tile runs
//    as before.  Rows >= M keep the limits of their row index on both sides: the lazy rescale is decided by a ballot over all
//    32 rows, and the bits of wave 0 of attn_i8_splitkv_causal_paged_window_kernel depend on it.
//  * The finish (dw_fused, set by the host iff num_splits == 1).  A 128-key window is two or three tiles, the split count is 1,
//    and the merge launch only adds q . km, applies the sink and rounds.  The epilogue then does that itself on the values it
//    holds, window_merge_row's operations for count == 1 in that function's order: the correction stays in a register instead
//    of being parked in the caller's lse, no partial is written, no workspace exists, and a workgroup of a sequence without keys
//    stores its rows' zeros and -inf before it returns.  No atomics and no order between workgroups: each owns its rows.
//    With more splits the kernel writes partials as the decode kernel does and window_merge_kernel merges them, unchanged.
//
// window, sinks and the flag travel beside the parameter block (DecodeWindowParams), so AttnParams keeps its layout.  Head_dim
// 128 with 16-bit P.V is at the end of the vector registers; a one-wave workgroup also has the accumulation registers, which
// the compiler takes for what the two-sided mask and the epilogue add.
#include <climits>
#include "../../include/sageattn_hip_decode_window.h"
#include "sage_attn_launch.h"

namespace sage {

struct DecodeWindowParams {
  AttnParams a;
  const float* sinks;  // fp32 [query heads of the un-folded view] or null
  int window;          // 1 .. a.N
  int fused_finish;    // one split: the epilogue finishes the rows, a.sk_o / a.sk_lse are null
};

template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
__global__ __launch_bounds__(64) void attn_i8_decode_paged_window_kernel(const DecodeWindowParams wp) {
  const AttnParams& p = wp.a;
  const int dw_window = wp.window;
  const float* const dw_sinks = wp.sinks;
  const bool dw_fused = wp.fused_finish != 0;
  constexpr bool PV_FP4 = false;
#define SAGE_ATTN_DECODE_BODY_OF_KERNEL
#define SAGE_ATTN_DECODE_BODY_WINDOW
#include "sage_attn_decode_body.h"
#undef SAGE_ATTN_DECODE_BODY_WINDOW
#undef SAGE_ATTN_DECODE_BODY_OF_KERNEL
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int launch_decode_window_attn(const AttnCall& c, const DecodeWindowParams& wp, hipStream_t st, int grid) {
  return by_dim(c.D, [&](auto d) {
    return by_flag(c.pv_fp8, [&](auto fp8) {
      constexpr int D = decltype(d)::value;
      constexpr bool PV_FP8 = decltype(fp8)::value;
      constexpr size_t smem = decode_lds_bytes(D, PV_FP8);
      return by_flag(c.kthread, [&](auto k) {
        return by_flag(c.v_bf16, [&](auto v) {
          void (*kern)(const DecodeWindowParams) =
              attn_i8_decode_paged_window_kernel<D, decltype(k)::value, !PV_FP8 && decltype(v)::value, PV_FP8>;
          if (!allow_lds((const void*)kern, smem)) return (int)SAGE_ERR_LAUNCH;
          hipLaunchKernelGGL(kern, dim3(grid), dim3(64), smem, st, wp);
          return launch_status();
        });
      });
    });
  });
}

// what attn_check sees in the place of the workspace of a one-split call, which has none: never dereferenced
alignas(16) static char no_workspace[16];

// The checks of decode_entry (sage_attn_decode.hip) and of window_entry (sage_attn_splitkv_window.hip) together; nothing is
// enqueued before every check has passed.
static int decode_window_entry(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                               const sage_tensor* o, int o_dtype, const float* k_scale, const void* km, bool pv_fp8,
                               const float* v_scale, float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq,
                               float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                               int num_pages, const int32_t* kv_lens, int num_splits, int q_fold, void* workspace,
                               size_t workspace_bytes, sage_stream_t stream, int window, const float* sinks) {
  if (window < 1 || ((uintptr_t)sinks & 3) || (sinks && !lse)) return SAGE_ERR_INVALID_ARGUMENT;
  if (pv_fp8 && !v_scale) return SAGE_ERR_INVALID_ARGUMENT;
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  if (page_size != 64 && page_size != 128 && page_size != 256) return SAGE_ERR_INVALID_ARGUMENT;
  if (!block_table || ((uintptr_t)block_table & 3) || !kv_lens || max_pages < 1 || num_pages < 1 || table_stride < max_pages ||
      table_stride > INT_MAX)
    return SAGE_ERR_INVALID_ARGUMENT;
  if ((int64_t)max_pages * page_size > INT_MAX) return SAGE_ERR_TOO_LARGE;
  if (M > kDecodeMaxRows) return SAGE_ERR_UNSUPPORTED;  // (more rows: sage_attn_fusedq_pv_*_splitkv_paged_window)
  const bool fused = num_splits == 1;                  // one launch, no workspace
  AttnArgs a;
  a.q = q; a.q_dtype = q_dtype; a.k8 = k8; a.v = v; a.v_dtype = v_dtype; a.o = o; a.o_dtype = o_dtype; a.k_scale = k_scale;
  a.km = km; a.v_scale = v_scale; a.pv_fp8 = pv_fp8; a.lse = lse;
  a.B = B; a.Hq = Hq; a.Hk = Hk; a.M = M; a.N = max_pages * page_size; a.D = D; a.qk_gran = qk_gran; a.blkq = 128; a.warpq = warpq;
  a.sm_scale = sm_scale;
  a.split_kv = true; a.split_kv_lens = kv_lens; a.num_splits = num_splits;
  a.split_workspace = fused ? (void*)no_workspace : workspace;
  a.split_workspace_bytes = fused ? (size_t)INT64_MAX : workspace_bytes;
  a.split_causal = true; a.q_fold = q_fold;
  a.paged = true; a.block_table = block_table; a.table_stride = (int)table_stride; a.page_size = page_size;
  AttnCall c;
  if (const int s = attn_check(c, a)) return s;
  if ((int64_t)B * Hq * num_splits > INT_MAX) return SAGE_ERR_TOO_LARGE;
  DecodeWindowParams wp;
  wp.a = c.p;
  wp.sinks = sinks;
  wp.window = window < a.N ? window : a.N;  // (a window beyond the capacity is the capacity: the limits then cannot overflow)
  wp.fused_finish = fused;
  if (fused) {
    wp.a.sk_o = nullptr;
    wp.a.sk_lse = nullptr;
  }
  const int s = launch_decode_window_attn(c, wp, (hipStream_t)stream, B * Hq * num_splits);
  if (s || fused) return s;
  return launch_window_merge(c, wp.window, sinks, (hipStream_t)stream);
}

}  // namespace sage

using namespace sage;

extern "C" int sage_attn_fusedq_pv_f16_decode_paged_window(
    const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool, const sage_tensor* v_pool, int v_dtype, const sage_tensor* o,
    int o_dtype, const float* k_scale_pool, const void* km, float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq,
    float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size, int num_pages,
    const int32_t* kv_lens, int num_splits, int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream, int window,
    const float* sinks) {
  return decode_window_entry(q, q_dtype, k8_pool, v_pool, v_dtype, o, o_dtype, k_scale_pool, km, false, nullptr, lse, B, Hq, Hk, M,
                             D, qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages, kv_lens,
                             num_splits, q_fold, workspace, workspace_bytes, stream, window, sinks);
}

extern "C" int sage_attn_fusedq_pv_f8_decode_paged_window(
    const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool, const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
    const float* k_scale_pool, const void* km, const float* v_scale, float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran,
    int warpq, float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size, int num_pages,
    const int32_t* kv_lens, int num_splits, int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream, int window,
    const float* sinks) {
  return decode_window_entry(q, q_dtype, k8_pool, v8_pool, SAGE_F16, o, o_dtype, k_scale_pool, km, true, v_scale, lse, B, Hq, Hk,
                             M, D, qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages, kv_lens,
                             num_splits, q_fold, workspace, workspace_bytes, stream, window, sinks);
}
