// Block-map predictor (SpargeAttn-style): which 128x64 tiles of a block-sparse attention call are
// worth computing, decided at run time from Q and K.
//   block_pool_sim_kernel   per block of BLK rows: the mean row and the mean pairwise cosine similarity ("self-similarity")
//                           of its rows.  One pass over the tensor, HBM-bound.
//   block_select_kernel     per (b, h_q, q-block): the pooled scores of the candidate key blocks (self-similar and not
//                           pinned on by keep_first / keep_last), then one of two rules -- CDF: the shortest descending
//                           prefix that holds cdfthreshd of their softmax mass; TOPK: the topk fraction of them with the
//                           greatest scores -- written as the tile list the block-sparse attention kernels read (and
//                           optionally as a map).
// Each kernel is one text with a template flag KVLEN for the forms with per-batch key lengths (sage_block_pool_sim_kvlen,
// sage_block_select_kvlen): `if constexpr (KVLEN)` at the few points where a length changes the walk, nothing of it in the
// instantiations without.
// The rule itself is stated in include/sageattn_hip.h.
#include "sage_entry.h"

namespace sage {

template <int CTRL>
__device__ __forceinline__ float dpp_lane_f(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
// sum over the TPR (8 or 16) consecutive lanes that hold one row.  Every step adds a lane's value to its partner's, so both
// partners -- and at the end all TPR lanes -- hold the same bits (a + b = b + a).
template <int TPR>
__device__ __forceinline__ float row_lanes_sum(float a) {
  static_assert(TPR == 8 || TPR == 16, "a row is 8 or 16 lanes");
  a += dpp_lane_f<0xB1>(a);   // quad_perm [1,0,3,2]
  a += dpp_lane_f<0x4E>(a);   // quad_perm [2,3,0,1]
  a += dpp_lane_f<0x141>(a);  // row_half_mirror: the other quad of the 8 lanes
  if constexpr (TPR == 16) a += dpp_lane_f<0x140>(a);  // row_mirror: the other half of the 16 lanes
  return a;
}
// xor butterflies over the wave: every lane ends with the same bits
__device__ __forceinline__ float wave_sum(float a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  return a;
}
__device__ __forceinline__ float wave_max(float a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
  return a;
}
__device__ __forceinline__ int wave_sum_i(int a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  return a;
}

// ------------------------------------------------------------------------------------------------
// block statistics
// ------------------------------------------------------------------------------------------------
struct PoolParams {
  const uint16_t* x;
  int64_t sb, sh, sn;
  const uint16_t* mean;  // [B,H,D] or null
  float* pooled;         // [B,H,nblk,D]
  float* sim;            // [B,H,nblk]
  int H, N, nblk;
  int per_wg, chunks;    // blocks per workgroup, workgroups per head
  const int32_t* kv_lens;  // KVLEN only (else null): int32 [B], batch b has the rows < clamp(kv_lens[b], 0, N)
};

// A workgroup walks per_wg consecutive blocks of one head.  D/8 threads hold a row (16 bytes each), 256/(D/8) rows per pass,
// BLK rows = NP loads per thread, all issued before the first use; the next block's rows are requested as soon as this
// block's are unpacked and fly during its reduction.  Rows past the end re-read the last row of the tensor (a valid address)
// and enter the sums through selects, so the ragged block costs no branch around a load.
// Summation order (fixed, so results are deterministic): a row's squared norm over the 8 channels of a thread and then
// over the row's lanes; a channel's sums over a thread's NP rows, then over the RPP thread rows in LDS; sim over the 64
// lanes of wave 0.  Zero rows (past the end, or a zero vector) add exact zeros.
// KVLEN (sage_block_pool_sim_kvlen): the same walk, with the end of batch b at its length len_b instead of N.  The grid and
// the output layout stay those of N.
template <int D, int BLK, bool BF16, bool KVLEN>
__global__ __launch_bounds__(256) void block_pool_sim_kernel(const PoolParams p) {
  constexpr int TPR = D / 8, RPP = 256 / TPR, NP = BLK / RPP;
  static_assert(NP >= 1, "block too small");
  __shared__ float red[2][RPP][D + 1];
  __shared__ float ssum[D];
  const int chunk = (int)(blockIdx.x % (unsigned)p.chunks);
  const int64_t bh = blockIdx.x / (unsigned)p.chunks;
  const int h = (int)(bh % p.H);
  const int64_t b = bh / p.H;
  const int tr = threadIdx.x / TPR, tc = threadIdx.x % TPR;
  const uint16_t* xbase = p.x + b * p.sb + h * p.sh + tc * 8;
  float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (p.mean) unpack8<BF16>(*reinterpret_cast<const uint4*>(p.mean + bh * D + tc * 8), m);
  int nrows = p.N;
  if constexpr (KVLEN) nrows = min(max(p.kv_lens[b], 0), p.N);  // len_b
  const int blk0 = chunk * p.per_wg;  // the host launches no empty workgroup
  int blk1 = min(blk0 + p.per_wg, p.nblk);
  if constexpr (KVLEN) {
    // the ragged block is the one that holds row len_b - 1, rows beyond it are never loaded (the row clamp goes to
    // len_b - 1), and the blocks wholly beyond it are left alone (workgroup uniform, in front of the first barrier;
    // len_b == 0: every workgroup of b)
    blk1 = min(blk1, (nrows + BLK - 1) / BLK);
    if (blk0 >= blk1) return;
  }
  const int last = nrows - 1;
  uint4 raw[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i)
    raw[i] = *reinterpret_cast<const uint4*>(xbase + (int64_t)min(blk0 * BLK + i * RPP + tr, last) * p.sn);
  for (int blk = blk0; blk < blk1; ++blk) {
    float f[NP][8];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      unpack8<BF16>(raw[i], f[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[i][j] -= m[j];
    }
    if (blk + 1 < blk1) {
#pragma unroll
      for (int i = 0; i < NP; ++i)
        raw[i] = *reinterpret_cast<const uint4*>(xbase + (int64_t)min((blk + 1) * BLK + i * RPP + tr, last) * p.sn);
    }
    float accx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, accu[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const bool valid = blk * BLK + i * RPP + tr <= last;
      float nsq = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) nsq = __builtin_fmaf(f[i][j], f[i][j], nsq);
      nsq = row_lanes_sum<TPR>(nsq);
      const float inv = valid && nsq > 0.f ? rsqrtf(nsq) : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        accx[j] += valid ? f[i][j] : 0.f;
        accu[j] = __builtin_fmaf(f[i][j], inv, accu[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[0][tr][tc * 8 + j] = accx[j];
      red[1][tr][tc * 8 + j] = accu[j];
    }
    __syncthreads();
    const int c = min(BLK, nrows - blk * BLK);
    const int64_t oblk = bh * p.nblk + blk;
    if (threadIdx.x < 2 * D) {  // the first D threads finish the mean, the next D the sum of unit rows
      const int which = threadIdx.x / D, d = threadIdx.x % D;
      float s = 0.f;
      for (int r = 0; r < RPP; ++r) s += red[which][r][d];  // fixed order
      if (which == 0) p.pooled[oblk * D + d] = s / (float)c;
      else ssum[d] = s;
    }
    __syncthreads();  // also: every read of `red` is done before the next block's writes
    if (threadIdx.x < 64) {
      float v = ssum[threadIdx.x] * ssum[threadIdx.x];
      if constexpr (D == 128) v = __builtin_fmaf(ssum[threadIdx.x + 64], ssum[threadIdx.x + 64], v);
      v = wave_sum(v);
      if (threadIdx.x == 0) p.sim[oblk] = v / (float)(c * c);
    }
    // wave 0 reads ssum before it arrives at the next block's first barrier; the others write it only behind that barrier
  }
}

// ------------------------------------------------------------------------------------------------
// selection
// ------------------------------------------------------------------------------------------------
struct SelectParams {
  const float *pq, *sq, *pk, *sk;  // [B,Hq,nqb,D], [B,Hq,nqb], [B,Hk,ntk,D], [B,Hk,ntk]
  const float *thr, *par;          // [Hq]: simthreshd1, and the rule's parameter (cdfthreshd or topk)
  int* lists;
  uint8_t* map;  // [B,Hq,nqb,ntk] or null
  int64_t rows;
  int Hq, Hk, nqb, ntk, row_ints;
  int kf, kl;  // key blocks j < kf and j >= ntk - kl are kept: always on, never candidates (both clamped to ntk)
  float sm_scale;
  const int32_t* kv_lens;  // KVLEN only (else null): int32 [B], batch b has ceil(clamp(kv_lens[b], 0, N) / 64) key blocks
};

// orders a wave's LDS writes before its own later reads of other lanes' words (one wave owns a row: no workgroup barrier)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A score as an unsigned key that orders like the score (-0 = +0), >= 1: 0 is left for the blocks that are no candidates.
__device__ __forceinline__ uint32_t score_key(float s) {
  const uint32_t u = __float_as_uint(s == 0.f ? 0.f : s);
  const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return key ? key : 1u;
}

// One wave per list row (b, h_q, q-block), four rows per workgroup (mostly q-blocks of one head: their reads of pooled K
// meet in the CU's cache); the row's p lives in the wave's quarter of LDS.
//  1. scores: 8 lanes per key block, each D/8 channels as float4 (a 128-byte run per 8 lanes), summed over the 8 lanes.
//     Only candidates (eligible, not kept) get one; the other blocks are forced on under either rule.
// RULE = SAGE_SELECT_CDF:
//  2. p = exp(s - max) over the candidates (the other blocks hold -1: negative as a float and as an int).
//  3. the prefix without a sort: p >= 0 orders like its bit pattern, so bisect on the pattern t for the largest t with
//     sum{p >= t} >= cdfthreshd * sum p (about 30 wave-reduced sums).  That t is one of the p; everything above it is
//     selected, and of the blocks equal to it the lowest indices, as many as the threshold still needs (one at least).
// RULE = SAGE_SELECT_TOPK: no softmax and no float sums.
//  2. the row holds score_key(s) for the candidates and 0 for the other blocks; n = count{key >= 1}, kcount from topk and n.
//  3. bisect on the key for the largest t with count{key >= t} >= kcount (32 counts, each ballots + popcounts: a value all
//     lanes hold).  Everything above t is selected, and of the keys equal to t the lowest indices, kcount - count{key > t}.
// Both:
//  4. emission as block_map_compact_kernel: ballot + prefix popcount, ascending, the tail padded with the last tile.
// Every sum runs in a fixed order and every decision is taken on values all lanes hold alike: deterministic, no atomics.
// KVLEN (sage_block_select_kvlen): the rule runs over the ntk_b = ceil(len_b / 64) key blocks of the row's batch instead of
// ntk -- kept blocks, candidates, n, kcount, the emission -- while every stride (pooled K, sim K, the LDS quarter, the list
// row, the map row) stays that of N.
template <int D, int RULE, bool KVLEN>
__global__ __launch_bounds__(256) void block_select_kernel(const SelectParams p) {
  static_assert(RULE == SAGE_SELECT_CDF || RULE == SAGE_SELECT_TOPK, "two rules");
  extern __shared__ float prow_all[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  if (row >= p.rows) return;
  float* prow = prow_all + (int64_t)w * p.ntk;
  const int64_t bh = row / p.nqb;
  const int hq = (int)(bh % p.Hq);
  const int64_t b = bh / p.Hq;
  const int64_t bhk = b * p.Hk + hq / (p.Hq / p.Hk);
  int ntk = p.ntk, kf = p.kf, kl = p.kl;
  if constexpr (KVLEN) {
    // ntk_b <= p.ntk (p.ntk << 6 >= N, and ceil(min(len, N) / 64) = ceil(min(len, 64 ntk) / 64))
    ntk = __builtin_amdgcn_readfirstlane((min(max(p.kv_lens[b], 0), (p.ntk << 6)) + 63) >> 6);
    kf = min(kf, ntk);
    kl = min(kl, ntk);
  }
  const float thr = p.thr[hq], par = p.par[hq];
  // a q-block that is not self-similar, or a cdfthreshd / topk of 1 and above (or NaN), keeps every tile
  bool all_on = !(p.sq[row] > thr) || !(par < 1.0f);
  if constexpr (KVLEN) all_on = all_on || ntk == 0;  // a batch without keys: nothing to score, and nothing is emitted below
  float mx = -INFINITY;
  uint32_t tbits = 0;
  int take = 0;
  if (!all_on) {
    const int sub = lane & 7, g = lane >> 3;
    const float* pk = p.pk + bhk * p.ntk * D;
    const float* sk = p.sk + bhk * p.ntk;
    float4 q4[D / 32];
#pragma unroll
    for (int i = 0; i < D / 32; ++i) q4[i] = *reinterpret_cast<const float4*>(p.pq + row * D + (i * 8 + sub) * 4);
    constexpr int U = 2;  // key blocks per lane group and step: all their loads are issued before the first use
    for (int j0 = 0; j0 < ntk; j0 += 8 * U) {
      float4 k4[U][D / 32];
      float skv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int jc = min(j0 + 8 * u + g, ntk - 1);  // past the end: the last block again, not stored
#pragma unroll
        for (int i = 0; i < D / 32; ++i) k4[u][i] = *reinterpret_cast<const float4*>(pk + (int64_t)jc * D + (i * 8 + sub) * 4);
        skv[u] = sk[jc];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + 8 * u + g;
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < D / 32; ++i) {
          dot = __builtin_fmaf(q4[i].x, k4[u][i].x, dot);
          dot = __builtin_fmaf(q4[i].y, k4[u][i].y, dot);
          dot = __builtin_fmaf(q4[i].z, k4[u][i].z, dot);
          dot = __builtin_fmaf(q4[i].w, k4[u][i].w, dot);
        }
        dot = row_lanes_sum<8>(dot);
        const bool cand = skv[u] > thr && j >= kf && j < ntk - kl;
        const float s = dot * p.sm_scale;
        if (sub == 0 && j < ntk) {
          if constexpr (RULE == SAGE_SELECT_TOPK) prow[j] = __uint_as_float(cand ? score_key(s) : 0u);
          else prow[j] = cand ? s : -INFINITY;
        }
      }
    }
    wave_lds_sync();
    if constexpr (RULE == SAGE_SELECT_CDF) {
      for (int j = lane; j < ntk; j += 64) mx = fmaxf(mx, prow[j]);
      mx = wave_max(mx);
      all_on = mx == -INFINITY;  // no candidate: every tile is forced on
    }
  }
  if constexpr (RULE == SAGE_SELECT_TOPK) {
    if (!all_on) {
      // candidates whose key is >= t (t >= 1), from ballots: the same value in every lane
      auto count_from = [&](uint32_t t) {
        int c = 0;
        for (int j0 = 0; j0 < ntk; j0 += 64) {
          const int j = j0 + lane;
          c += __popcll(__ballot(j < ntk && __float_as_uint(prow[j]) >= t));
        }
        return c;
      };
      const int n = count_from(1u);
      all_on = n == 0;  // no candidate: every tile is forced on
      if (!all_on) {
        const float want = ceilf(par * (float)n);  // one fp32 product; par < 1 here
        const int kcount = want >= (float)n ? n : want > 1.f ? (int)want : 1;
        uint64_t lo = 1, hi = 1ull << 32;  // count_from(lo) >= kcount > count_from(hi): no key is 2^32
        while (hi - lo > 1) {
          const uint64_t mid = lo + ((hi - lo) >> 1);
          if (count_from((uint32_t)mid) >= kcount) lo = mid; else hi = mid;
        }
        tbits = (uint32_t)lo;  // one of the keys; hi = lo + 1
        take = kcount - (hi < (1ull << 32) ? count_from((uint32_t)hi) : 0);
      }
    }
  } else if (!all_on) {
    float tot = 0.f;
    for (int j = lane; j < ntk; j += 64) {  // each lane rewrites the words it read
      const float s = prow[j];
      const float pj = s == -INFINITY ? -1.0f : expf(s - mx);
      prow[j] = pj;
      tot += fmaxf(pj, 0.f);
    }
    wave_lds_sync();
    const float target = par * wave_sum(tot);
    // sum of the p whose pattern is >= t, in the order of `tot`: skipped terms add exact zeros
    auto mass_from = [&](int t) {
      float gsum = 0.f;
      for (int j = lane; j < ntk; j += 64) {
        const float pj = prow[j];
        gsum += __float_as_int(pj) >= t ? pj : 0.f;
      }
      return wave_sum(gsum);
    };
    int lo = 0, hi = 0x3F800001;  // mass_from(lo) >= target; no p is above 1.0f
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if (mass_from(mid) >= target) lo = mid; else hi = mid;
    }
    tbits = (uint32_t)lo;
    const float tstar = __int_as_float(lo);
    const float above = mass_from(lo + 1);
    int nties = 0;
    for (int j = lane; j < ntk; j += 64) nties += __float_as_int(prow[j]) == lo ? 1 : 0;
    nties = wave_sum_i(nties);
    take = 1;
    if (tstar > 0.f) {
      const float need = ceilf((target - above) / tstar);
      take = need >= (float)nties ? nties : need > 1.f ? (int)need : 1;
      if (take > 1 && above + (float)(take - 1) * tstar >= target) --take;
      if (take < nties && above + (float)take * tstar < target) ++take;
    }
  }
  int* out = p.lists + row * p.row_ints;
  uint8_t* mrow = p.map ? p.map + row * p.ntk : nullptr;
  int count = 0, lastj = 0, ties_before = 0;
  for (int j0 = 0; j0 < ntk; j0 += 64) {
    const int j = j0 + lane;
    const bool in = j < ntk;
    bool on = in;
    if (!all_on) {
      const uint32_t pb = in ? __float_as_uint(prow[j]) : 0u;
      const bool tie = in && pb == tbits;
      const uint64_t tbal = __ballot(tie);
      const int rank = ties_before + __popcll(tbal & ((1ull << lane) - 1ull));
      ties_before += __popcll(tbal);
      // forced on: the blocks that are no candidates hold -1.0f (CDF) or the key 0 (TOPK)
      const bool forced = RULE == SAGE_SELECT_TOPK ? pb == 0u : (int)pb < 0;
      const bool above = RULE == SAGE_SELECT_TOPK ? pb > tbits : (int)pb > (int)tbits;
      on = in && (forced || above || (tie && rank < take));
    }
    const uint64_t bal = __ballot(on);
    if (on) out[1 + count + __popcll(bal & ((1ull << lane) - 1ull))] = j;
    if (mrow && in) mrow[j] = on ? 1 : 0;
    count += __popcll(bal);
    if (bal) lastj = j0 + 63 - __clzll((long long)bal);
  }
  for (int i = 1 + count + lane; i < p.row_ints; i += 64) out[i] = lastj;
  if (lane == 0) out[0] = count;
  if constexpr (KVLEN) {  // map columns >= ntk_b are written 0 (with ntk_b == 0 the list above is empty)
    if (mrow)
      for (int j = ntk + lane; j < p.ntk; j += 64) mrow[j] = 0;
  }
}

// Blocks per workgroup of the pooling kernel: as many as leave about `target` workgroups for all B*H heads.
static int blocks_per_wg(int64_t BH, int nblk, int64_t target) {
  const int64_t per = (BH * nblk + target - 1) / target;
  return (int)(per < 1 ? 1 : per > nblk ? nblk : per);
}

}  // namespace sage

using namespace sage;

// sage_block_pool_sim and its twin with per-batch lengths (kvlen: kv_lens is required)
static int block_pool_sim(const sage_tensor* x, int dtype, int B, int H, int N, int D, int blk, const void* mean,
                          float* pooled, float* sim, bool kvlen, const int32_t* kv_lens, sage_stream_t stream) {
  if (kvlen && (!kv_lens || ((uintptr_t)kv_lens & 3))) return SAGE_ERR_INVALID_ARGUMENT;
  if (!tensor_ok(x, 8) || !pooled || !sim || !aligned16(pooled) || B <= 0 || H <= 0 || N <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = dim_dtype_status(D, dtype)) return s;
  if (blk != 64 && blk != 128) return SAGE_ERR_INVALID_ARGUMENT;
  if (mean && !aligned16(mean)) return SAGE_ERR_INVALID_ARGUMENT;
  PoolParams p;
  p.x = (const uint16_t*)x->data; p.sb = x->stride_b; p.sh = x->stride_h; p.sn = x->stride_n;
  p.mean = (const uint16_t*)mean; p.pooled = pooled; p.sim = sim; p.kv_lens = kv_lens;
  p.H = H; p.N = N; p.nblk = (int)(((int64_t)N + blk - 1) / blk);
  // eight resident workgroups per CU stream their share of a head each
  p.per_wg = blocks_per_wg((int64_t)B * H, p.nblk, 256 * 8);
  p.chunks = (p.nblk + p.per_wg - 1) / p.per_wg;
  const int64_t grid = (int64_t)B * H * p.chunks;
  if (grid >= ((int64_t)1 << 31)) return SAGE_ERR_TOO_LARGE;
  launch_begin();
  by_dim(D, [&](auto d) {
    by_flag(blk == 128, [&](auto big) {
      by_flag(dtype == SAGE_BF16, [&](auto bf) {
        by_flag(kvlen, [&](auto len) {
          constexpr int DD = decltype(d)::value, BLK = decltype(big)::value ? 128 : 64;
          constexpr bool BF = decltype(bf)::value, KVLEN = decltype(len)::value;
          hipLaunchKernelGGL((block_pool_sim_kernel<DD, BLK, BF, KVLEN>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p);
        });
      });
    });
  });
  return launch_status();
}

extern "C" int sage_block_pool_sim(const sage_tensor* x, int dtype, int B, int H, int N, int D, int blk, const void* mean,
                                   float* pooled, float* sim, sage_stream_t stream) {
  return block_pool_sim(x, dtype, B, H, N, D, blk, mean, pooled, sim, false, nullptr, stream);
}

extern "C" int sage_block_pool_sim_kvlen(const sage_tensor* x, int dtype, int B, int H, int N, int D, int blk, const void* mean,
                                         float* pooled, float* sim, const int32_t* kv_lens, sage_stream_t stream) {
  return block_pool_sim(x, dtype, B, H, N, D, blk, mean, pooled, sim, true, kv_lens, stream);
}

// sage_block_select and its twin with per-batch lengths (kvlen: kv_lens is required)
static int block_select(const float* pooled_q, const float* sim_q, const float* pooled_k, const float* sim_k,
                        int B, int Hq, int Hk, int M, int N, int D, float sm_scale, const float* simthreshd1,
                        int rule, const float* rule_param, int keep_first, int keep_last, int32_t* block_lists,
                        int64_t block_lists_bytes, uint8_t* block_map, bool kvlen, const int32_t* kv_lens,
                        sage_stream_t stream) {
  if (kvlen && (!kv_lens || ((uintptr_t)kv_lens & 3))) return SAGE_ERR_INVALID_ARGUMENT;
  if (!pooled_q || !sim_q || !pooled_k || !sim_k || !simthreshd1 || !rule_param || !block_lists) return SAGE_ERR_INVALID_ARGUMENT;
  if (!aligned16(pooled_q) || !aligned16(pooled_k) || !aligned16(block_lists)) return SAGE_ERR_INVALID_ARGUMENT;
  if (B <= 0 || Hq <= 0 || Hk <= 0 || Hq % Hk != 0 || M <= 0 || N <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (rule != SAGE_SELECT_CDF && rule != SAGE_SELECT_TOPK) return SAGE_ERR_INVALID_ARGUMENT;
  if (keep_first < 0 || keep_last < 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (D != 64 && D != 128) return SAGE_ERR_UNSUPPORTED_HEAD_DIM;
  if (!(sm_scale > 0.f) || !(sm_scale < INFINITY)) return SAGE_ERR_INVALID_ARGUMENT;
  if (((int64_t)N + 63) / 64 > SAGE_SPARGE_MAX_KEY_TILES) return SAGE_ERR_TOO_LARGE;  // the rows of a workgroup in LDS
  if (block_lists_bytes < block_sparse_bytes(B, Hq, M, N)) return SAGE_ERR_INVALID_ARGUMENT;
  SelectParams p;
  p.pq = pooled_q; p.sq = sim_q; p.pk = pooled_k; p.sk = sim_k; p.thr = simthreshd1; p.par = rule_param;
  p.lists = (int*)block_lists; p.map = block_map;
  p.Hq = Hq; p.Hk = Hk; p.nqb = (M + 127) / 128; p.ntk = (N + 63) / 64; p.row_ints = (int)block_list_row(N);
  p.kf = keep_first < p.ntk ? keep_first : p.ntk; p.kl = keep_last < p.ntk ? keep_last : p.ntk;
  p.rows = (int64_t)B * Hq * p.nqb;
  p.sm_scale = sm_scale; p.kv_lens = kv_lens;
  if ((p.rows + 3) / 4 >= ((int64_t)1 << 31)) return SAGE_ERR_TOO_LARGE;
  launch_begin();
  by_dim(D, [&](auto d) {
    by_flag(rule == SAGE_SELECT_TOPK, [&](auto topk) {
      by_flag(kvlen, [&](auto len) {
        constexpr int DD = decltype(d)::value, RULE = decltype(topk)::value ? SAGE_SELECT_TOPK : SAGE_SELECT_CDF;
        const dim3 grid((unsigned)((p.rows + 3) / 4));
        const size_t lds = (size_t)4 * p.ntk * sizeof(float);
        hipLaunchKernelGGL((block_select_kernel<DD, RULE, decltype(len)::value>), grid, dim3(256), lds, (hipStream_t)stream, p);
      });
    });
  });
  return launch_status();
}

extern "C" int sage_block_select(const float* pooled_q, const float* sim_q, const float* pooled_k, const float* sim_k,
                                 int B, int Hq, int Hk, int M, int N, int D, float sm_scale, const float* simthreshd1,
                                 int rule, const float* rule_param, int keep_first, int keep_last, int32_t* block_lists,
                                 int64_t block_lists_bytes, uint8_t* block_map, sage_stream_t stream) {
  return block_select(pooled_q, sim_q, pooled_k, sim_k, B, Hq, Hk, M, N, D, sm_scale, simthreshd1, rule, rule_param, keep_first,
                      keep_last, block_lists, block_lists_bytes, block_map, false, nullptr, stream);
}

extern "C" int sage_block_select_kvlen(const float* pooled_q, const float* sim_q, const float* pooled_k, const float* sim_k,
                                       int B, int Hq, int Hk, int M, int N, int D, float sm_scale, const float* simthreshd1,
                                       int rule, const float* rule_param, int keep_first, int keep_last, int32_t* block_lists,
                                       int64_t block_lists_bytes, uint8_t* block_map, const int32_t* kv_lens,
                                       sage_stream_t stream) {
  return block_select(pooled_q, sim_q, pooled_k, sim_k, B, Hq, Hk, M, N, D, sm_scale, simthreshd1, rule, rule_param, keep_first,
                      keep_last, block_lists, block_lists_bytes, block_map, true, kv_lens, stream);
}

extern "C" int sage_block_select_cdf(const float* pooled_q, const float* sim_q, const float* pooled_k, const float* sim_k,
                                     int B, int Hq, int Hk, int M, int N, int D, float sm_scale, const float* simthreshd1,
                                     const float* cdfthreshd, int32_t* block_lists, int64_t block_lists_bytes,
                                     uint8_t* block_map, sage_stream_t stream) {
  return sage_block_select(pooled_q, sim_q, pooled_k, sim_k, B, Hq, Hk, M, N, D, sm_scale, simthreshd1, SAGE_SELECT_CDF,
                           cdfthreshd, 0, 0, block_lists, block_lists_bytes, block_map, stream);
}
