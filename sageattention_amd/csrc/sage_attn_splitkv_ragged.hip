// Ragged-query attention on the paged KV cache (the rule: include/sageattn_hip_ragged.h): the causal paged split-KV kernel for
// a mixed batch whose queries are packed, q [total_tokens, Hq, D] with cu_seqlens_q.  Three kernels:
//
//  * ragged_q_plan_kernel: one workgroup scans ceil(T_b * g / 128) over the sequences and writes the work list, one pair
//    (b, qb) per 128-row q-block that exists.  A batch that is mostly decode then costs a workgroup per sequence and split, not
//    B x max-q-blocks of them.
//  * attn_i8_splitkv_causal_paged_ragged_kernel: sage_attn_body.h with CAUSAL, SPLITKV, PAGED and the macro
//    SAGE_ATTN_BODY_RAGGED.  A workgroup is (work item, head, split); M_ is the sequence's own T_b * g, the diagonal offset
//    len_b - T_b, and the fused Q quantizer forms its row address as (cu[b] + r / g) * token stride + (h * g + r % g) * head
//    stride, so the fold of the GQA group into rows costs no copy.  Everything else -- tile copies through per-tile
//    descriptors, page ids an iteration ahead, masks, lazy rescale, partial stores -- is the existing text.
//  * ragged_merge_kernel: walks the same list (no token-to-sequence search), derives the split count of the q-block as
//    splitkv_merge_kernel<CAUSAL = true> does, uses its arithmetic in split order and stores o and lse at the un-folded
//    addresses [token, hk * g + i].
//
// A kernel of its own name and a source file of its own, as every other twin: the build's guards match kernels by name, and
// the other instantiations keep their code and their registers.
#include <climits>
#include "../../include/sageattn_hip_ragged.h"
#include "sage_attn_launch.h"

namespace sage {

// ---- the work list -----------------------------------------------------------------------------------------------------------
// 256 sequences per round: thread t counts the q-blocks of sequence c0 + t, an inclusive scan over the workgroup (Hillis-Steele
// in LDS) turns the counts into offsets, and the threads then write the round's pairs together -- pair i of the round belongs to
// the sequence whose offset range holds i, found by bisection in LDS -- so that one prefill chunk of many q-blocks is not one
// thread's loop.  `carry`, the pairs of the rounds before, is the same value in every thread.  Nothing is written at or beyond
// n_items, whatever cu holds; the slots behind the last pair get b = -1.
__global__ __launch_bounds__(256) void ragged_q_plan_kernel(const int32_t* __restrict__ cu, const int B, const int total_tokens,
                                                            const int g, int32_t* __restrict__ items, const int n_items) {
  __shared__ int off[2][256];
  __shared__ int start[257];
  const int tid = threadIdx.x;
  int carry = 0;
  for (int c0 = 0; c0 < B; c0 += 256) {
    const int b = c0 + tid;
    int n = 0;
    if (b < B) {
      const int T = min(max(cu[b + 1] - cu[b], 0), total_tokens);  // (T * g <= total_tokens * g, which the host holds below 2^31)
      n = min((int)(((int64_t)T * g + 127) >> 7), n_items);
    }
    int cur = 0;
    off[0][tid] = n;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int v = off[cur][tid] + (tid >= d ? off[cur][tid - d] : 0);
      off[cur ^ 1][tid] = v;
      cur ^= 1;
      __syncthreads();
    }
    const int incl = off[cur][tid];
    start[tid + 1] = incl;
    if (tid == 0) start[0] = 0;
    __syncthreads();
    const int cnt = min(start[256], n_items - carry);    // (n <= n_items and n_items <= INT_MAX / 256: the sums cannot overflow)
    for (int i = tid; i < cnt; i += 256) {
      int lo = 0, hi = 255;  // the last s with start[s] <= i
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= i) lo = mid; else hi = mid - 1;
      }
      *reinterpret_cast<int2*>(items + 2 * (int64_t)(carry + i)) = make_int2(c0 + lo, i - start[lo]);
    }
    carry += cnt;
    __syncthreads();
  }
  for (int i = carry + tid; i < n_items; i += 256) *reinterpret_cast<int2*>(items + 2 * (int64_t)i) = make_int2(-1, 0);
}

// ---- the attention kernel ----------------------------------------------------------------------------------------------------
template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
// (register budget as attn_i8_kernel: head_dim 64 FP8 PV with 4 waves is held to three waves per SIMD)
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_splitkv_causal_paged_ragged_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = true, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true, PAGED = true;
#define SAGE_ATTN_BODY_OF_KERNEL
#define SAGE_ATTN_BODY_RAGGED
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_RAGGED
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// ---- the merge -----------------------------------------------------------------------------------------------------------------
// One workgroup per (work item, head, run of 256 / (D / 4) rows of the q-block), one thread per 4 output channels of a row.
// The sequence's bounds are clamped exactly as the attention kernel clamps them, and count, mx, sum and acc are those of
// splitkv_merge_kernel<.., CAUSAL = true> (sage_attn_splitkv.hip) with M = T_b * g -- the same operations in the same order, so
// the row has that merge's bits.  What differs is where things live: the partial slots by packed row, o and lse un-folded.
template <bool BF16, int MAXC>
__global__ __launch_bounds__(256) void ragged_merge_kernel(const AttnParams p, const int D) {
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
  const int ntk_b = (len_b + 63) >> 6, tps_b = (ntk_b + p.num_splits - 1) / p.num_splits;
  // the count of splits of the row's q-block (see splitkv_merge_kernel): end_qb is the key bound of its last row < M
  const int tok = min((m | 127), M - 1) / g;
  const int end_qb = min(len_b, (tok - T) + len_b + 1);
  const int count = end_qb > 0 ? min((ntk_b + tps_b - 1) / tps_b, (((end_qb + 63) >> 6) + tps_b - 1) / tps_b) : 0;
  const int t = m / g, i = m - t * g;
  const int64_t token = q_lo + t;
  const int head = h * g + i;
  uint16_t* const op = p.o + token * p.osn + head * p.osh + c * 4;
  float* const lp = p.lse ? p.lse + token * ((int64_t)p.Hq * g) + head : nullptr;
  if (count == 0) {  // no split ran: o = 0, lse = -inf; nothing of the workspace (or of the parked correction) is read
    *reinterpret_cast<uint2*>(op) = make_uint2(0u, 0u);
    if (c == 0 && lp) *lp = -INFINITY;
    return;
  }
  const int64_t rows = (int64_t)p.Hq * p.M;                                  // rows of one split's slots
  const int64_t row = (int64_t)h * p.M + (int64_t)q_lo * g + m;
  float l[MAXC];
  float4 raw[MAXC];
#pragma unroll
  for (int k = 0; k < MAXC; ++k) {
    const int s = k < count ? k : count - 1;
    l[k] = p.sk_lse[(int64_t)s * rows + row];
    raw[k] = *reinterpret_cast<const float4*>(p.sk_o + ((int64_t)s * rows + row) * D + c * 4);
  }
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
  uint2 w2;
  w2.x = (uint32_t)f32_to_elem_bits<BF16>(acc[0] * inv) | ((uint32_t)f32_to_elem_bits<BF16>(acc[1] * inv) << 16);
  w2.y = (uint32_t)f32_to_elem_bits<BF16>(acc[2] * inv) | ((uint32_t)f32_to_elem_bits<BF16>(acc[3] * inv) << 16);
  *reinterpret_cast<uint2*>(op) = w2;
  if (c == 0 && lp) {
    // natural log of the merged base-2 LSE, then the correction q . km that split 0 parked in the slot; product and sum rounded
    // separately, as in splitkv_merge_kernel
#pragma clang fp contract(off)
    float v = (sum > 0.f ? mx + log2f(sum) : -INFINITY) / 1.44269504f;
    v += *lp * p.sm_scale;
    *lp = v;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// n_items of a call, or -1 where it (or the packed row count) leaves the range the kernels index with int
static int64_t ragged_items(int B, int total_tokens, int q_fold) {
  const int64_t rows = (int64_t)total_tokens * q_fold;
  if (rows > INT_MAX) return -1;
  const int64_t n = rows / 128 + B;
  return n > INT_MAX / 256 ? -1 : n;
}

static int ragged_entry(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                        const sage_tensor* o, int o_dtype, const float* k_scale, const void* km, bool pv_fp8,
                        const float* v_scale, float* lse, int B, int Hq, int Hk, int total_tokens, int D, int qk_gran, int warpq,
                        float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                        int num_pages, const int32_t* kv_lens, const int32_t* cu, const int32_t* items, int n_items,
                        int num_splits, int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  if (pv_fp8 && !v_scale) return SAGE_ERR_INVALID_ARGUMENT;
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  if (page_size != 64 && page_size != 128 && page_size != 256) return SAGE_ERR_INVALID_ARGUMENT;
  if (!block_table || ((uintptr_t)block_table & 3) || !kv_lens || max_pages < 1 || num_pages < 1 || table_stride < max_pages ||
      table_stride > INT_MAX)
    return SAGE_ERR_INVALID_ARGUMENT;
  if (B <= 0 || Hq <= 0 || Hk <= 0 || Hq % Hk != 0 || total_tokens < 1) return SAGE_ERR_INVALID_ARGUMENT;
  if (q_fold != 1 && q_fold != Hq / Hk) return SAGE_ERR_INVALID_ARGUMENT;
  if (!cu || ((uintptr_t)cu & 3) || !items || ((uintptr_t)items & 7) || !q || !o) return SAGE_ERR_INVALID_ARGUMENT;
  if ((int64_t)max_pages * page_size > INT_MAX) return SAGE_ERR_TOO_LARGE;
  const int64_t want = ragged_items(B, total_tokens, q_fold);
  if (want < 0) return SAGE_ERR_TOO_LARGE;
  if (n_items != want) return SAGE_ERR_INVALID_ARGUMENT;
  const int Hf = Hq / q_fold;
  if ((int64_t)n_items * Hf * num_splits > INT_MAX || (int64_t)n_items * Hf * (D / 8) > INT_MAX) return SAGE_ERR_TOO_LARGE;
  // The folded view as ONE batch of Hq / g heads and total_tokens * g rows: attn_check then checks what the paged causal
  // entry checks, sizes the workspace [S, Hq / g, total_tokens * g] and fills the parameters; stride_b is not read.
  const sage_tensor qv = {q->data, 0, q->stride_h, q->stride_n}, ov = {o->data, 0, o->stride_h, o->stride_n};
  AttnArgs a;
  a.q = &qv; a.q_dtype = q_dtype; a.k8 = k8; a.v = v; a.v_dtype = v_dtype; a.o = &ov; a.o_dtype = o_dtype; a.k_scale = k_scale;
  a.km = km; a.v_scale = v_scale; a.pv_fp8 = pv_fp8; a.lse = lse;
  a.B = 1; a.Hq = Hf; a.Hk = Hk; a.M = total_tokens * q_fold; a.N = max_pages * page_size; a.D = D; a.qk_gran = qk_gran;
  a.blkq = 128; a.warpq = warpq; a.sm_scale = sm_scale;
  a.split_kv = true; a.split_kv_lens = kv_lens; a.num_splits = num_splits; a.split_workspace = workspace;
  a.split_workspace_bytes = workspace_bytes;
  a.split_causal = true; a.q_fold = q_fold;
  a.paged = true; a.block_table = block_table; a.table_stride = (int)table_stride; a.page_size = page_size;
  AttnCall c;
  if (const int s = attn_check(c, a)) return s;
  // ... then what is the ragged form's own (the words of cu_q, v_mean and nqb; B counts the sequences again)
  c.p.B = B; c.p.cu_q = cu; c.p.rq_items = items; c.p.nqb = n_items;
  hipStream_t st = (hipStream_t)stream;
  const int s = launch_4wave_kernel(c, st, n_items * Hf * num_splits, [](auto d, auto k, auto vb, auto fp8) {
    return attn_i8_splitkv_causal_paged_ragged_kernel<decltype(d)::value, decltype(k)::value, decltype(vb)::value,
                                                      decltype(fp8)::value>;
  });
  if (s) return s;
  by_flag(c.p.out_bf16 != 0, [&](auto bf) {
    by_slots(num_splits, [&](auto slots) {
      hipLaunchKernelGGL((ragged_merge_kernel<decltype(bf)::value, decltype(slots)::value>), dim3((unsigned)(n_items * Hf * (D / 8))),
                         dim3(256), 0, st, c.p, D);
    });
  });
  return launch_status();
}

}  // namespace sage

using namespace sage;

extern "C" int sage_ragged_q_plan(const int32_t* cu_seqlens_q, int B, int total_tokens, int q_fold, int32_t* items, int n_items,
                                  sage_stream_t stream) {
  if (B < 1 || total_tokens < 1 || q_fold < 1 || !cu_seqlens_q || ((uintptr_t)cu_seqlens_q & 3) || !items ||
      ((uintptr_t)items & 7))
    return SAGE_ERR_INVALID_ARGUMENT;
  const int64_t want = ragged_items(B, total_tokens, q_fold);
  if (want < 0) return SAGE_ERR_TOO_LARGE;
  if (n_items != want) return SAGE_ERR_INVALID_ARGUMENT;
  launch_begin();
  hipLaunchKernelGGL(ragged_q_plan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, cu_seqlens_q, B, total_tokens, q_fold, items,
                     n_items);
  return launch_status();
}

extern "C" size_t sage_ragged_workspace_bytes(int total_tokens, int Hq, int D, int num_splits) {
  if (total_tokens <= 0 || Hq <= 0 || D <= 0 || num_splits < 1 || num_splits > SAGE_MERGE_MAX) return 0;
  return (size_t)splitkv_bytes(1, Hq, total_tokens, D, num_splits);
}

extern "C" int sage_attn_fusedq_pv_f16_splitkv_paged_ragged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                            const sage_tensor* v_pool, int v_dtype, const sage_tensor* o,
                                                            int o_dtype, const float* k_scale_pool, const void* km, float* lse,
                                                            int B, int Hq, int Hk, int total_tokens, int D, int qk_gran,
                                                            int warpq, float sm_scale, const int32_t* block_table,
                                                            int64_t table_stride, int max_pages, int page_size, int num_pages,
                                                            const int32_t* kv_lens, const int32_t* cu_seqlens_q,
                                                            const int32_t* items, int n_items, int num_splits, int q_fold,
                                                            void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  return ragged_entry(q, q_dtype, k8_pool, v_pool, v_dtype, o, o_dtype, k_scale_pool, km, false, nullptr, lse, B, Hq, Hk,
                      total_tokens, D, qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages,
                      kv_lens, cu_seqlens_q, items, n_items, num_splits, q_fold, workspace, workspace_bytes, stream);
}

extern "C" int sage_attn_fusedq_pv_f8_splitkv_paged_ragged(const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool,
                                                           const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
                                                           const float* k_scale_pool, const void* km, const float* v_scale,
                                                           float* lse, int B, int Hq, int Hk, int total_tokens, int D,
                                                           int qk_gran, int warpq, float sm_scale, const int32_t* block_table,
                                                           int64_t table_stride, int max_pages, int page_size, int num_pages,
                                                           const int32_t* kv_lens, const int32_t* cu_seqlens_q,
                                                           const int32_t* items, int n_items, int num_splits, int q_fold,
                                                           void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  return ragged_entry(q, q_dtype, k8_pool, v8_pool, SAGE_F16, o, o_dtype, k_scale_pool, km, true, v_scale, lse, B, Hq, Hk,
                      total_tokens, D, qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages,
                      kv_lens, cu_seqlens_q, items, n_items, num_splits, q_fold, workspace, workspace_bytes, stream);
}
