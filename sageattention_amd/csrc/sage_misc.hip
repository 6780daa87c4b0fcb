// Small helpers of the hot path: library info, LSE finishing (core.py:651) and the ring-attention
// state merge (new component; rule in SURVEY.md section 5).  Elementwise, HBM-bound.
#include "sage_entry.h"

namespace sage {

template <bool BF16>
__global__ __launch_bounds__(256) void merge_states_kernel(float* __restrict__ o_acc, float* __restrict__ lse_acc,
                                                           const uint16_t* __restrict__ o_blk,
                                                           const float* __restrict__ lse_blk, int64_t rows, int D) {
  // one thread per 8 output elements; D/8 threads per row
  const int tpr = D / 8;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = gid / tpr;
  const int c = (int)(gid % tpr);
  if (row >= rows) return;
  const float la = lse_acc[row], lb = lse_blk[row];
  const float mx = fmaxf(la, lb);
  // logaddexp; la = -inf (empty accumulator) gives wa = 0, wb = 1
  const bool use_a = la != -INFINITY, use_b = lb != -INFINITY;
  const float ea = use_a ? __expf(la - mx) : 0.f, eb = use_b ? __expf(lb - mx) : 0.f;
  const float sum = ea + eb;
  const float lse = (sum > 0.f) ? mx + __logf(sum) : -INFINITY;
  const float wa = (sum > 0.f) ? ea / sum : 0.f, wb = (sum > 0.f) ? eb / sum : 0.f;
  float* oa = o_acc + row * D + c * 8;
  float fb[8];
  unpack8<BF16>(*reinterpret_cast<const uint4*>(o_blk + row * D + c * 8), fb);
  const float4 a0 = *reinterpret_cast<float4*>(oa), a1 = *reinterpret_cast<float4*>(oa + 4);
  const float fa[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  // an empty side's o may hold anything (a torch.empty accumulator, the o of a fully masked block): its contribution is
  // taken by a select, as in merge_many_kernel -- NaN * 0 would poison the row
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (use_a ? fa[j] : 0.f) * wa + (use_b ? fb[j] : 0.f) * wb;
  *reinterpret_cast<float4*>(oa) = make_float4(r[0], r[1], r[2], r[3]);
  *reinterpret_cast<float4*>(oa + 4) = make_float4(r[4], r[5], r[6], r[7]);
  __syncthreads();  // all threads of a row have read lse_acc[row] (rows never straddle a block: 256 % tpr == 0)
  if (c == 0) lse_acc[row] = lse;
}

// Multi-way merge: (o, lse) = merge of up to SAGE_MERGE_MAX block results in ONE pass -- a ring step over P shards
// otherwise reads and writes the fp32 accumulator P times (sage_merge_attn_states per block).
struct MergeMany {
  const uint16_t* o[SAGE_MERGE_MAX];
  const float* lse[SAGE_MERGE_MAX];
  int count;
};
// MAXC: compile-time bound of `count` (2, 4, 8 or 16): the slots are unrolled
template <bool BF16, int MAXC>
__global__ __launch_bounds__(256) void merge_many_kernel(const MergeMany m, uint16_t* __restrict__ o_out,
                                                         float* __restrict__ lse_out, int64_t rows, int D,
                                                         const float in_mult, const float* __restrict__ corr,
                                                         const float corr_mult) {
  const int tpr = D / 8;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = gid / tpr;
  const int c = (int)(gid % tpr);
  if (row >= rows) return;
  // every lse and every o row of this thread is requested up front (slots unrolled; a slot past `count` repeats the last
  // one and is not used): as a run-time loop with the o load under `if (l != -inf)` each block cost two dependent round
  // trips -- hipcc sinks a load into the branch that uses it.  The uses below are selects, not branches, for that reason.
  // The combination runs in slot order: deterministic, bit-identical.
  float l[MAXC];
  uint4 raw[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int s = i < m.count ? i : m.count - 1;
    {
      // the scaled LSE is rounded ONCE: contracted into `l[i] - mx` below (an fma), the maximum's own exponent argument is
      // the product's rounding residue instead of 0, and a lone or dominant block's LSE comes back one ulp off
#pragma clang fp contract(off)
      l[i] = m.lse[s][row] * in_mult;
    }
    raw[i] = *reinterpret_cast<const uint4*>(m.o[s] + row * D + c * 8);
  }
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) mx = i < m.count ? fmaxf(mx, l[i]) : mx;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {  // fixed order: deterministic
    const bool use = i < m.count && l[i] != -INFINITY;  // empty block (e.g. fully masked): weight 0, its o may be anything
    const float w = __expf(l[i] - mx);
    sum = use ? sum + w : sum;
    float f[8];
    unpack8<BF16>(raw[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = use ? acc[j] + f[j] * w : acc[j];
  }
  const float inv = sum > 0.f ? 1.0f / sum : 0.f;
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    w[j] = (uint32_t)f32_to_elem_bits<BF16>(acc[2 * j] * inv) | ((uint32_t)f32_to_elem_bits<BF16>(acc[2 * j + 1] * inv) << 16);
  *reinterpret_cast<uint4*>(o_out + row * D + c * 8) = make_uint4(w[0], w[1], w[2], w[3]);
  if (c == 0 && lse_out) lse_out[row] = (sum > 0.f ? mx + __logf(sum) : -INFINITY) + (corr ? corr[row] * corr_mult : 0.f);
}

__global__ __launch_bounds__(256) void finish_lse_kernel(const float* __restrict__ lse2, const float* __restrict__ corr,
                                                         float sm_scale, float* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  // product and sum rounded separately, as torch evaluates core.py:651 and as the fused-Q epilogue of the attention kernel
  // does (sage_attn.hip is built with -ffp-contract=off): contracted to an fma, this kernel and that epilogue differed in the
  // last bit whenever sm_scale is not a power of two (head_dim 128), although both are documented as bit-identical
  {
#pragma clang fp contract(off)
    float v = lse2[i] / 1.44269504f;  // core.py:651
    if (corr) v += corr[i] * sm_scale;
    out[i] = v;
  }
}

// Block map -> per-(b, h, q-block) lists of active 64-key tiles (the operand of the block-sparse attention kernels).  One
// wave per list row: 64 map entries per step, ballot + prefix popcount give every active tile its slot, so the list ascends
// and the result is deterministic (no atomics).  The rest of the row is filled with the last active tile (kBlockListPad
// entries at least): the attention loop reads ahead of the list's end without a clamp.
__global__ __launch_bounds__(256) void block_map_compact_kernel(const uint8_t* __restrict__ map, int64_t sb, int64_t sh,
                                                                int64_t si, int64_t sj, int64_t rows, int Hq, int nqb,
                                                                int ntk, int row_ints, int* __restrict__ lists) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int qb = (int)(row % nqb);
  const int64_t bh = row / nqb;
  const uint8_t* m = map + (bh / Hq) * sb + (bh % Hq) * sh + qb * si;
  int* out = lists + row * row_ints;
  int count = 0, last = 0;
  for (int j0 = 0; j0 < ntk; j0 += 64) {
    const int j = j0 + lane;
    const bool on = j < ntk && m[(int64_t)j * sj] != 0;
    const uint64_t bal = __ballot(on);
    if (on) out[1 + count + __popcll(bal & ((1ull << lane) - 1ull))] = j;
    count += __popcll(bal);
    if (bal) last = j0 + 63 - __clzll((long long)bal);
  }
  for (int i = 1 + count + lane; i < row_ints; i += 64) out[i] = last;
  if (lane == 0) out[0] = count;
}

int finish_lse_check(FinishLseCall& c, const float* lse2, const float* corr, float sm_scale, float* lse_out, int64_t n) {
  if (!lse2 || !lse_out || n <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  c = FinishLseCall{lse2, corr, sm_scale, lse_out, n};
  return SAGE_OK;
}

int finish_lse_launch(const FinishLseCall& c, hipStream_t st) {
  launch_begin();
  hipLaunchKernelGGL(finish_lse_kernel, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, st, c.lse2, c.corr, c.sm_scale,
                     c.out, c.n);
  return launch_status();
}

}  // namespace sage

using namespace sage;

extern "C" int sage_abi_version(void) { return SAGEATTN_HIP_ABI_VERSION; }
extern "C" const char* sage_target_arch(void) { return "gfx950"; }
extern "C" const char* sage_status_string(int status) {
  switch (status) {
    case SAGE_OK: return "ok";
    case SAGE_ERR_INVALID_ARGUMENT: return "invalid argument (null/unaligned pointer, bad enum or inconsistent sizes)";
    case SAGE_ERR_UNSUPPORTED_HEAD_DIM: return "unsupported head_dim (must be 64 or 128 after padding)";
    case SAGE_ERR_UNSUPPORTED: return "configuration not supported by this build";
    case SAGE_ERR_TOO_LARGE: return "tensor slice too large";
    case SAGE_ERR_LAUNCH: return "HIP kernel launch failed";
    default: return "unknown status";
  }
}

extern "C" int sage_merge_attn_states(float* o_acc, float* lse_acc, const void* o_blk, int o_dtype, const float* lse_blk,
                                      int64_t rows, int D, sage_stream_t stream) {
  if (!o_acc || !lse_acc || !o_blk || !lse_blk || rows <= 0 || !aligned16(o_acc) || !aligned16(o_blk)) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = dim_dtype_status(D, o_dtype)) return s;
  const int64_t threads = rows * (D / 8);
  launch_begin();
  by_flag(o_dtype == SAGE_BF16, [&](auto bf) {
    hipLaunchKernelGGL((merge_states_kernel<decltype(bf)::value>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, o_acc, lse_acc, (const uint16_t*)o_blk, lse_blk, rows, D);
  });
  return launch_status();
}

// merge_many_kernel's slot count as a compile-time constant: the first of 2, 4, 8, 16 that holds `count`
template <class F>
static void by_slots(int count, F&& f) {
  if (count <= 2) f(std::integral_constant<int, 2>{});
  else if (count <= 4) f(std::integral_constant<int, 4>{});
  else if (count <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

extern "C" int sage_merge_attn_states_multi_ex(const void* const* o_blks, const float* const* lse_blks, int count, int o_dtype,
                                               void* o_out, float* lse_out, int64_t rows, int D, float lse_in_mult,
                                               const float* corr, float corr_mult, sage_stream_t stream) {
  if (!(lse_in_mult > 0.f)) return SAGE_ERR_INVALID_ARGUMENT;
  if (!o_blks || !lse_blks || !o_out || count <= 0 || count > SAGE_MERGE_MAX || rows <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = dim_dtype_status(D, o_dtype)) return s;
  MergeMany m;
  m.count = count;
  for (int i = 0; i < count; ++i) {
    if (!o_blks[i] || !lse_blks[i] || !aligned16(o_blks[i])) return SAGE_ERR_INVALID_ARGUMENT;
    m.o[i] = (const uint16_t*)o_blks[i];
    m.lse[i] = lse_blks[i];
  }
  for (int i = count; i < SAGE_MERGE_MAX; ++i) { m.o[i] = nullptr; m.lse[i] = nullptr; }
  if (!aligned16(o_out)) return SAGE_ERR_INVALID_ARGUMENT;
  const int64_t threads = rows * (D / 8);
  launch_begin();
  by_flag(o_dtype == SAGE_BF16, [&](auto bf) {
    by_slots(count, [&](auto slots) {
      hipLaunchKernelGGL((merge_many_kernel<decltype(bf)::value, decltype(slots)::value>), dim3((unsigned)((threads + 255) / 256)),
                         dim3(256), 0, (hipStream_t)stream, m, (uint16_t*)o_out, lse_out, rows, D, lse_in_mult, corr, corr_mult);
    });
  });
  return launch_status();
}

extern "C" int sage_merge_attn_states_multi(const void* const* o_blks, const float* const* lse_blks, int count, int o_dtype,
                                           void* o_out, float* lse_out, int64_t rows, int D, sage_stream_t stream) {
  return sage_merge_attn_states_multi_ex(o_blks, lse_blks, count, o_dtype, o_out, lse_out, rows, D, 1.0f, nullptr, 0.f, stream);
}

extern "C" size_t sage_block_sparse_workspace_bytes(int B, int Hq, int M, int N) {
  if (B <= 0 || Hq <= 0 || M <= 0 || N <= 0) return 0;
  return (size_t)block_sparse_bytes(B, Hq, M, N);
}

extern "C" int sage_block_map_compact(const void* block_map, const int64_t* map_strides, int B, int Hq, int M, int N,
                                      int32_t* block_lists, int64_t block_lists_bytes, sage_stream_t stream) {
  if (!block_map || !map_strides || !block_lists || !aligned16(block_lists)) return SAGE_ERR_INVALID_ARGUMENT;
  if (B <= 0 || Hq <= 0 || M <= 0 || N <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < 4; ++i)
    if (map_strides[i] < 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (block_lists_bytes < block_sparse_bytes(B, Hq, M, N)) return SAGE_ERR_INVALID_ARGUMENT;
  const int nqb = (M + 127) / 128, ntk = (N + 63) / 64;
  const int64_t rows = (int64_t)B * Hq * nqb;
  if ((rows + 3) / 4 >= ((int64_t)1 << 31)) return SAGE_ERR_TOO_LARGE;
  launch_begin();
  hipLaunchKernelGGL(block_map_compact_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)block_map, map_strides[0], map_strides[1], map_strides[2], map_strides[3], rows, Hq, nqb,
                     ntk, (int)block_list_row(N), (int*)block_lists);
  return launch_status();
}

extern "C" int sage_finish_lse(const float* lse2, const float* corr, float sm_scale, float* lse_out, int64_t n,
                               sage_stream_t stream) {
  FinishLseCall c;
  if (const int s = finish_lse_check(c, lse2, corr, sm_scale, lse_out, n)) return s;
  return finish_lse_launch(c, (hipStream_t)stream);
}
