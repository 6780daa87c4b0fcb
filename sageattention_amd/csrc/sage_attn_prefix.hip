// Shared-prefix attention on the paged KV cache (the rule: include/sageattn_hip_prefix.h).  The prefix is a sequence of its
// own with its own frozen statistics; a call runs attn_i8_splitkv_paged_kernel (sage_attn_splitkv_paged.hip) on the prefix with
// the B sequences' query rows folded into the rows of one batch -- the prefix K / V leave HBM once for all of them --, then
// attn_i8_splitkv_causal_paged_kernel (sage_attn_splitkv_causal_paged.hip) on the suffixes as it stands, then the one kernel
// of this file: prefix_merge_kernel, which merges the splits of each segment by the arithmetic of splitkv_merge_kernel
// (sage_attn_splitkv.hip) and combines the two segments.  The raw base-2 LSEs of the attention kernels lack q . km_seg and km
// differs per segment, so each segment's correction enters its weight before the two are combined; splitkv_merge_kernel adds
// one correction, once, at the end.  The attention loop (sage_attn_body.h) is not touched.
//
// Contraction is off for the whole file (the build's flags): the LSE tail rounds product and sum separately, as the other
// merges do.
#include <climits>
#include "../../include/sageattn_hip_prefix.h"
#include "sage_attn_launch.h"

namespace sage {

struct PrefixMergeParams {
  // per segment: the partial outputs fp32 [S, rows, D], their raw base-2 LSEs fp32 [S, rows], the q . km_seg that split 0 parked
  // fp32 [rows]; rows = B * Hq * M, in the prefix pass's order [Hq, B * M] for p and in q's order [B, Hq, M] for s
  const float *p_o, *p_lse, *p_corr;
  const float *s_o, *s_lse, *s_corr;
  const int32_t* prefix_len;  // int32 [1]
  const int32_t* kv_lens;     // int32 [B]: the suffix lengths
  int Np, Ns;                 // logical capacities of the two tables
  int Sp, Ss;                 // splits of the two passes
  int B, Hq, M, q_fold;
  float sm_scale;
  uint16_t* o; int64_t osb, osh, osn;
  float* lse;                 // fp32 [B, Hq, M] or null
};

// the slots < count of one row: every lse and every o run requested up front, slots unrolled (the comment on
// splitkv_merge_kernel), and the parked correction with them; a slot index past the count repeats the last valid one.
// Called with count > 0 only: with count 0 nothing of the segment's workspace was written by this call and nothing is read.
template <int MAXC>
__device__ __forceinline__ void prefix_seg_load(const float* sk_o, const float* sk_lse, const float* corr_p, int64_t rows,
                                                int64_t row, int D, int c, int count, float (&l)[MAXC], float4 (&raw)[MAXC],
                                                float& corr) {
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int s = i < count ? i : count - 1;
    l[i] = sk_lse[(int64_t)s * rows + row];
    raw[i] = *reinterpret_cast<const float4*>(sk_o + ((int64_t)s * rows + row) * D + c * 4);
  }
  corr = corr_p[row];
}

// round_to_dtype(a * b) as splitkv_merge_kernel rounds its output elements.  For fp16 hipcc makes that kernel's product and
// rounding ONE instruction with one rounding, v_fma_mixlo_f16; here the same product also exists as the fp32 o_x, the compiler
// shares the multiply and converts its fp32 result -- two roundings, and an ulp off that kernel's bits in one element of a few
// thousand.  So the instruction is spelled out.  bf16 has no such form: the product is rounded to fp32 there as here.
template <bool BF16>
__device__ __forceinline__ uint16_t round_product(float a, float b) {
  if constexpr (BF16) {
    return f32_to_elem_bits<true>(a * b);
  } else {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r = 0;  // (the instruction writes the low half of its destination and keeps the high one)
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "+v"(r) : "v"(a), "v"(b));
    return (uint16_t)r;
#else
    return f32_to_elem_bits<false>(a * b);
#endif
  }
}

// the merge of one segment's splits: mx, sum and acc as splitkv_merge_kernel forms them, in split order with the same
// selects; then o_x = acc * (1 / sum) and L_x, the natural-log LSE with the segment's own correction in it (the operations of
// that kernel's LSE tail), -inf where the segment has no key for the row.  alone: the output elements of the segment on its
// own, as that kernel rounds them (round_product)
template <bool BF16, int MAXC>
__device__ __forceinline__ void prefix_seg_merge(const float (&l)[MAXC], const float4 (&raw)[MAXC], int count, float corr,
                                                 float sm_scale, float (&o)[4], uint16_t (&alone)[4], float& L) {
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
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = acc[j] * inv;
    alone[j] = round_product<BF16>(acc[j], inv);
  }
  {
#pragma clang fp contract(off)
    float v = (sum > 0.f ? mx + log2f(sum) : -INFINITY) / 1.44269504f;
    v += corr * sm_scale;
    L = sum > 0.f ? v : -INFINITY;
  }
}

// The merge of a shared-prefix call.  One thread per 4 output channels of a row (b, h, m): it reads the prefix slots at the
// folded row h * (B * M) + b * M + m and the suffix slots at the native row (b * Hq + h) * M + m, and makes one 8-byte store of
// o in q's layout -- the un-fold costs nothing.  MAXP / MAXS: compile-time bounds of the two split counts (2, 4, 8 or 16).
template <bool BF16, int MAXP, int MAXS>
__global__ __launch_bounds__(256) void prefix_merge_kernel(const PrefixMergeParams p, const int D) {
  const int tpr = D / 4;
  const int64_t rows = (int64_t)p.B * p.Hq * p.M;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = gid / tpr;
  const int c = (int)(gid % tpr);
  if (row >= rows) return;
  const int m = (int)(row % p.M);
  const int64_t bh = row / p.M;
  const int h = (int)(bh % p.Hq), b = (int)(bh / p.Hq);
  const int64_t prow = ((int64_t)h * p.B + b) * p.M + m;  // the row of the prefix pass: [Hq, B * M]
  // the counts, exactly as splitkv_merge_kernel derives them: non-causal with B = 1 for the prefix ...
  const int len_p = min(max(p.prefix_len[0], 0), p.Np);
  const int ntk_p = (len_p + 63) >> 6, tps_p = (ntk_p + p.Sp - 1) / p.Sp;
  const int count_p = tps_p > 0 ? (ntk_p + tps_p - 1) / tps_p : 0;
  // ... and the causal count of the row's q-block for the suffix
  const int len_b = min(max(p.kv_lens[b], 0), p.Ns);
  const int ntk_b = (len_b + 63) >> 6, tps_b = (ntk_b + p.Ss - 1) / p.Ss;
  const int tok = min((m | 127), p.M - 1) / p.q_fold;
  const int end_qb = min(len_b, (tok - p.M / p.q_fold) + len_b + 1);
  const int count_s = end_qb > 0 ? min((ntk_b + tps_b - 1) / tps_b, (((end_qb + 63) >> 6) + tps_b - 1) / tps_b) : 0;

  float lp[MAXP], ls[MAXS];
  float4 rp[MAXP], rs[MAXS];
  float corr_p = 0.f, corr_s = 0.f;
  if (count_p > 0) {
    prefix_seg_load<MAXP>(p.p_o, p.p_lse, p.p_corr, rows, prow, D, c, count_p, lp, rp, corr_p);
  } else {
#pragma unroll
    for (int i = 0; i < MAXP; ++i) { lp[i] = -INFINITY; rp[i] = make_float4(0.f, 0.f, 0.f, 0.f); }
  }
  if (count_s > 0) {
    prefix_seg_load<MAXS>(p.s_o, p.s_lse, p.s_corr, rows, row, D, c, count_s, ls, rs, corr_s);
  } else {
#pragma unroll
    for (int i = 0; i < MAXS; ++i) { ls[i] = -INFINITY; rs[i] = make_float4(0.f, 0.f, 0.f, 0.f); }
  }
  float o_p[4], o_s[4], L_p, L_s;
  uint16_t a_p[4], a_s[4];
  prefix_seg_merge<BF16, MAXP>(lp, rp, count_p, corr_p, p.sm_scale, o_p, a_p, L_p);
  prefix_seg_merge<BF16, MAXS>(ls, rs, count_s, corr_s, p.sm_scale, o_s, a_s, L_s);

  // combine, prefix then suffix; a segment without a key for the row is dropped by a select, never multiplied by zero.  With
  // one segment alone w = expf(0) = 1 and 1 / 1 = 1: lse is that segment's L_x, and o the segment's own rounding (`alone`)
  const float mx = fmaxf(L_p, L_s);
  const bool use_p = L_p != -INFINITY, use_s = L_s != -INFINITY;
  const float w_p = expf(L_p - mx), w_s = expf(L_s - mx);
  float sum = 0.f;
  sum = use_p ? sum + w_p : sum;
  sum = use_s ? sum + w_s : sum;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc[j] = use_p ? acc[j] + o_p[j] * w_p : acc[j];
    acc[j] = use_s ? acc[j] + o_s[j] * w_s : acc[j];
  }
  const float inv = sum > 0.f ? 1.0f / sum : 0.f;  // a row without any key: o = 0, lse = -inf
  uint16_t* const op = p.o + b * p.osb + h * p.osh + (int64_t)m * p.osn + c * 4;
  uint16_t e[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint16_t both = f32_to_elem_bits<BF16>(acc[j] * inv);
    e[j] = (use_p && use_s) ? both : use_p ? a_p[j] : use_s ? a_s[j] : (uint16_t)0;
  }
  uint2 w2;
  w2.x = (uint32_t)e[0] | ((uint32_t)e[1] << 16);
  w2.y = (uint32_t)e[2] | ((uint32_t)e[3] << 16);
  *reinterpret_cast<uint2*>(op) = w2;
  if (c == 0 && p.lse) p.lse[row] = sum > 0.f ? mx + logf(sum) : -INFINITY;
}

// the merge launch of a shared-prefix call: the slots and the parked corrections are where the two attention calls put them
int launch_prefix_merge(const AttnCall& prefix, const AttnCall& suffix, float* lse, hipStream_t st) {
  const AttnParams& pp = prefix.p;
  const AttnParams& ps = suffix.p;
  PrefixMergeParams m;
  m.p_o = pp.sk_o; m.p_lse = pp.sk_lse; m.p_corr = pp.lse;
  m.s_o = ps.sk_o; m.s_lse = ps.sk_lse; m.s_corr = ps.lse;
  m.prefix_len = pp.kv_lens; m.kv_lens = ps.kv_lens;
  m.Np = pp.N; m.Ns = ps.N; m.Sp = pp.num_splits; m.Ss = ps.num_splits;
  m.B = ps.B; m.Hq = ps.Hq; m.M = ps.M; m.q_fold = ps.q_fold; m.sm_scale = ps.sm_scale;
  m.o = ps.o; m.osb = ps.osb; m.osh = ps.osh; m.osn = ps.osn;
  m.lse = lse;
  const int D = suffix.D;
  const int64_t threads = (int64_t)m.B * m.Hq * m.M * (D / 4);
  by_flag(ps.out_bf16 != 0, [&](auto bf) {
    by_slots(m.Sp, [&](auto sp) {
      by_slots(m.Ss, [&](auto ss) {
        hipLaunchKernelGGL((prefix_merge_kernel<decltype(bf)::value, decltype(sp)::value, decltype(ss)::value>),
                           dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, m, D);
      });
    });
  });
  return launch_status();
}

// A shared-prefix entry point.  What is its own is checked here; the rest by attn_check on the two segments' argument blocks
// -- the suffix block is that of splitkv_paged_entry (sage_attn_splitkv_paged.hip) with causal set, the prefix block the
// non-causal one with B = 1, M = B * M and a q whose stride_n walks the folded rows.  Nothing is enqueued before every check
// has passed.
//
// The workspace, sage_prefix_workspace_bytes in all: [prefix o slots | suffix o slots | prefix LSE slots | suffix LSE slots |
// prefix correction | suffix correction].  Both o regions are whole 16-byte units (D * 4 bytes per row), which the 16-byte
// loads and stores of the slots need; the LSE slots of a split-KV call behind its own o slots would leave the second call's
// o slots on a 4-byte boundary whenever S * rows is odd.  So each call is checked on the bytes from its o slots to the end
// -- never fewer than it asks for -- and its sk_lse is then moved to its region.
static int prefix_entry(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                        const sage_tensor* o, int o_dtype, const float* k_scale, const void* km, bool pv_fp8,
                        const float* v_scale, float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran, int warpq,
                        float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                        int num_pages, const int32_t* kv_lens, const int32_t* prefix_table, int max_prefix_pages,
                        const int32_t* prefix_len, const void* km_p, const float* v_scale_p, int prefix_splits, int num_splits,
                        int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  if (pv_fp8 && (!v_scale || !v_scale_p)) return SAGE_ERR_INVALID_ARGUMENT;
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  if (page_size != 64 && page_size != 128 && page_size != 256) return SAGE_ERR_INVALID_ARGUMENT;
  if (!block_table || ((uintptr_t)block_table & 3) || !kv_lens || max_pages < 1 || num_pages < 1 || table_stride < max_pages ||
      table_stride > INT_MAX)
    return SAGE_ERR_INVALID_ARGUMENT;
  if (!prefix_table || ((uintptr_t)prefix_table & 3) || !prefix_len || ((uintptr_t)prefix_len & 3) || max_prefix_pages < 1)
    return SAGE_ERR_INVALID_ARGUMENT;
  if (B <= 0 || Hq <= 0 || M <= 0 || D <= 0 || prefix_splits < 1 || prefix_splits > SAGE_MERGE_MAX || num_splits < 1 ||
      num_splits > SAGE_MERGE_MAX || !tensor_ok(q, 8) || !workspace)
    return SAGE_ERR_INVALID_ARGUMENT;
  if ((int64_t)max_pages * page_size > INT_MAX || (int64_t)max_prefix_pages * page_size > INT_MAX || (int64_t)B * M > INT_MAX)
    return SAGE_ERR_TOO_LARGE;
  // the folded q: row b * M + m of the one batch is q[b, h, m]
  sage_tensor qp = *q;
  if (M == 1) qp.stride_n = B > 1 ? q->stride_b : q->stride_n;
  else if (B > 1 && q->stride_b != (int64_t)M * q->stride_n) return SAGE_ERR_UNSUPPORTED;
  const int64_t rows = (int64_t)B * Hq * M;
  float* const ws = (float*)workspace;
  float* const o_s = ws + (int64_t)prefix_splits * rows * D;
  float* const lse_p = o_s + (int64_t)num_splits * rows * D;
  float* const lse_s = lse_p + (int64_t)prefix_splits * rows;
  float* const corr_p = lse_s + (int64_t)num_splits * rows;
  float* const corr_s = corr_p + rows;
  const size_t before_s = (size_t)((char*)o_s - (char*)ws);

  AttnArgs s;  // the suffixes: the causal paged call
  s.q = q; s.q_dtype = q_dtype; s.k8 = k8; s.v = v; s.v_dtype = v_dtype; s.o = o; s.o_dtype = o_dtype; s.k_scale = k_scale;
  s.km = km; s.v_scale = v_scale; s.pv_fp8 = pv_fp8; s.lse = corr_s;
  s.B = B; s.Hq = Hq; s.Hk = Hk; s.M = M; s.N = max_pages * page_size; s.D = D; s.qk_gran = qk_gran; s.blkq = 128; s.warpq = warpq;
  s.sm_scale = sm_scale;
  s.split_kv = true; s.split_kv_lens = kv_lens; s.num_splits = num_splits; s.split_workspace = o_s;
  s.split_workspace_bytes = workspace_bytes > before_s ? workspace_bytes - before_s : 0;
  s.split_causal = true; s.q_fold = q_fold;
  s.paged = true; s.block_table = block_table; s.table_stride = (int)table_stride; s.page_size = page_size;
  AttnArgs p = s;  // the prefix: the non-causal paged call on one batch of B * M rows
  p.q = &qp; p.km = km_p; p.v_scale = v_scale_p; p.lse = corr_p;
  p.B = 1; p.M = B * M; p.N = max_prefix_pages * page_size;
  p.split_kv_lens = prefix_len; p.num_splits = prefix_splits; p.split_workspace = workspace;
  p.split_workspace_bytes = workspace_bytes;
  p.split_causal = false; p.q_fold = 1;
  p.block_table = prefix_table; p.table_stride = max_prefix_pages;
  AttnCall cs, cp;
  if (const int st = attn_check(cs, s)) return st;
  if (const int st = attn_check(cp, p)) return st;
  if (workspace_bytes < sage_prefix_workspace_bytes(B, Hq, M, D, prefix_splits, num_splits)) return SAGE_ERR_INVALID_ARGUMENT;
  cp.p.sk_lse = lse_p;
  cs.p.sk_lse = lse_s;
  if (const int st = launch_splitkv_paged_attn(cp, (hipStream_t)stream)) return st;
  if (const int st = launch_splitkv_causal_paged_attn(cs, (hipStream_t)stream)) return st;
  return launch_prefix_merge(cp, cs, lse, (hipStream_t)stream);
}

}  // namespace sage

using namespace sage;

extern "C" size_t sage_prefix_workspace_bytes(int B, int Hq, int M, int D, int prefix_splits, int num_splits) {
  if (B <= 0 || Hq <= 0 || M <= 0 || D <= 0 || prefix_splits < 1 || prefix_splits > SAGE_MERGE_MAX || num_splits < 1 ||
      num_splits > SAGE_MERGE_MAX || (int64_t)B * M > INT_MAX)
    return 0;
  return (size_t)(splitkv_bytes(1, Hq, B * M, D, prefix_splits) + splitkv_bytes(B, Hq, M, D, num_splits) +
                  2 * (int64_t)B * Hq * M * 4);
}

extern "C" int sage_attn_fusedq_pv_f16_splitkv_paged_prefix(
    const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool, const sage_tensor* v_pool, int v_dtype, const sage_tensor* o,
    int o_dtype, const float* k_scale_pool, const void* km, float* lse, int B, int Hq, int Hk, int M, int D, int qk_gran,
    int warpq, float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size, int num_pages,
    const int32_t* kv_lens, const int32_t* prefix_table, int max_prefix_pages, const int32_t* prefix_len, const void* km_p,
    int prefix_splits, int num_splits, int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream) {
  return prefix_entry(q, q_dtype, k8_pool, v_pool, v_dtype, o, o_dtype, k_scale_pool, km, false, nullptr, lse, B, Hq, Hk, M, D,
                      qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages, kv_lens,
                      prefix_table, max_prefix_pages, prefix_len, km_p, nullptr, prefix_splits, num_splits, q_fold, workspace,
                      workspace_bytes, stream);
}

extern "C" int sage_attn_fusedq_pv_f8_splitkv_paged_prefix(
    const sage_tensor* q, int q_dtype, const sage_tensor* k8_pool, const sage_tensor* v8_pool, const sage_tensor* o, int o_dtype,
    const float* k_scale_pool, const void* km, const float* v_scale, float* lse, int B, int Hq, int Hk, int M, int D,
    int qk_gran, int warpq, float sm_scale, const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
    int num_pages, const int32_t* kv_lens, const int32_t* prefix_table, int max_prefix_pages, const int32_t* prefix_len,
    const void* km_p, const float* v_scale_p, int prefix_splits, int num_splits, int q_fold, void* workspace,
    size_t workspace_bytes, sage_stream_t stream) {
  return prefix_entry(q, q_dtype, k8_pool, v8_pool, SAGE_F16, o, o_dtype, k_scale_pool, km, true, v_scale, lse, B, Hq, Hk, M, D,
                      qk_gran, warpq, sm_scale, block_table, table_stride, max_pages, page_size, num_pages, kv_lens,
                      prefix_table, max_prefix_pages, prefix_len, km_p, v_scale_p, prefix_splits, num_splits, q_fold, workspace,
                      workspace_bytes, stream);
}
