// Calibration of the block-map predictor: what a block map loses, measured on the operands the
// attention kernels multiply.
//   tile_mass_kernel     per (b, h_q, 128-row q-block): the softmax mass of every 64-key tile, exact -- the probabilities of the
//                        dense operator summed over the tile's keys and averaged over the q-block's valid rows.  Two passes over
//                        the key tiles: row maximum and row sum, then the normalised probabilities.  QK^T only, no P.V.
//   plan_recall_kernel   per list row of a plan: the sum of that mass over the tiles the list keeps, and their number.
// The definitions are stated in include/sageattn_hip.h.  Neither kernel uses atomics; every sum runs in a fixed order.
// Each kernel is one text with a trailing template flag KVLEN for the forms with per-batch key lengths (sage_attn_tile_mass_kvlen,
// sage_block_plan_recall_kvlen), as the predictor's kernels are (sage_sparge.hip): `if constexpr (KVLEN)` at the few points
// where a length changes something, nothing of it in the instantiations without lengths, and kv_lens the last member of the
// parameter block (null without lengths).
#include "sage_entry.h"

namespace sage {
namespace {

template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
// sum over the 64 lanes, the same tree in every call: quads, the 8 and the 16 lanes of a DPP row, then the rows
__device__ __forceinline__ float wave_sum_fixed(float a) {
  a += dpp_f<0xB1>(a);   // quad_perm [1,0,3,2]
  a += dpp_f<0x4E>(a);   // quad_perm [2,3,0,1]
  a += dpp_f<0x141>(a);  // row_half_mirror
  a += dpp_f<0x140>(a);  // row_mirror
  a += __shfl_xor(a, 16);
  a += __shfl_xor(a, 32);
  return a;
}
// orders a wave's LDS writes before its own later reads of other lanes' words (one wave owns its words: no workgroup barrier)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float exp2_raw(float x) {  // v_exp_f32: x <= 0 here, -inf gives exactly 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_exp2f(x);
#else
  return 0.f;
#endif
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// exact tile mass
// ------------------------------------------------------------------------------------------------
struct MassParams {
  const int8_t* q; int64_t qsb, qsh, qsn;
  const int8_t* k; int64_t ksb, ksh, ksn;
  const float* q_scale;
  const float* k_scale;
  float* mass;  // [B,Hq,nqb,ntk]
  int Hq, Hk, M, N;
  int nqb, ntk;
  int gq, gk;   // scales per (b,h)
  int qgran, blkq, warpq;
  float logit_mult;
  int B;                   // KVLEN only: the workgroup ids are split head-major
  const int32_t* kv_lens;  // KVLEN only (else null): int32 [B], batch b has the keys < clamp(kv_lens[b], 0, N)
};

// One workgroup of 4 waves per (q-block, h, b), 32 query rows per wave, the geometry of the attention kernels: S^T = K . Q^T
// by v_mfma_i32_32x32x32_i8 with the Q fragments resident, lane (r, hh) holding query row r and, per 32-key half mt of a
// tile, the keys 32 mt + (e & 3) + 8 (e >> 2) + 4 hh of registers e = 0..15 (sage_attn_body.h).  The K tile is staged through
// LDS in the body's image (16-byte chunk XOR k_swz) with plain 16-byte loads, the next tile's chunks in flight during this
// tile's arithmetic; rows past the end re-read row N - 1 (a valid address) and are masked.
//   logit   t = float(S) * (q_scale(r) * logit_mult * k_scale(n)), v_cvt_f32_i32 exact (|S| <= 128 * 127^2 < 2^24); keys >= N
//           become -inf, so exp2 gives exactly 0.
//   pass 1  per lane and tile: the maximum of its 32 logits, the rescaled sum l = l * 2^(m - m') + sum 2^(t - m'); at the end
//           the two lane halves of a row are merged: m = max, l = l_a 2^(m_a - m) + l_b 2^(m_b - m) (spelled without
//           contraction, so both lanes of a row hold the same bits).
//   pass 2  p = 2^(t - m) / l; the lane's 32 values by a pairwise tree, 0 for a row >= M, then wave_sum_fixed; the four
//           waves' numbers meet in LDS and thread 0 adds them in wave order, divides by the q-block's valid rows and stores
//           the entry -- while the workgroup is already at the next tile.
// Every entry of the q-block's row of `mass` is written; a wave whose rows are all >= M contributes an exact 0 and skips the
// arithmetic (it still stages K and meets every barrier).
// KVLEN (sage_attn_tile_mass_kvlen): the same two sweeps over the ntk_b = ceil(len_b / 64) tiles of the batch, len_b read with
// one scalar load, so everything derived from it is workgroup uniform.  Rows are clamped to len_b - 1 and the tail mask sits
// in tile ntk_b - 1 against len_b: neither a K row >= len_b nor the scales of a tile >= ntk_b are ever loaded.  Pass 1 adds
// tiles in ascending order and pass 2 works tile by tile, so the entries < ntk_b have the bits of the kernel without lengths
// on the slice of the first len_b keys; the entries [ntk_b, ntk) are stored as 0 behind the second sweep.  A batch without
// keys has no row len_b - 1 to clamp to: its workgroups zero their row and leave before any load of K and any barrier.  The
// workgroup ids are split head-major as in attn_i8_kvlen_kernel (batches alternate within a head, so that no XCD holds only
// the longest batch), and the row of `mass` is addressed by (b, h, q-block).
template <int D, bool KTHREAD, bool KVLEN>
__global__ __launch_bounds__(256) void tile_mass_kernel(const MassParams p) {
  constexpr int KS = D / 32;              // k-steps of the int8 MFMA
  constexpr int KCH = D / 16;             // 16-B chunks per K row
  constexpr int KC = (64 * KCH) / 256;    // chunks per thread and tile
  static_assert(KC * 256 == 64 * KCH, "a K tile divides over the workgroup");
  __shared__ __attribute__((aligned(16))) char k_lds[64 * D];
  __shared__ float wpart[4];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int qb = (int)(blockIdx.x % (unsigned)p.nqb);
  const int bh = (int)(blockIdx.x / (unsigned)p.nqb);
  const int h = KVLEN ? bh / p.B : bh % p.Hq, b = KVLEN ? bh % p.B : bh / p.Hq;
  const int hk = h / (p.Hq / p.Hk);
  int nkeys = p.N, ntk = p.ntk;  // the batch's keys and key tiles
  float* mrow = p.mass + (int64_t)blockIdx.x * p.ntk;
  if constexpr (KVLEN) {
    nkeys = min(max(uniform_load_i32(p.kv_lens + b), 0), p.N);  // len_b
    ntk = (nkeys + 63) >> 6;                                    // ntk_b
    mrow = p.mass + (((int64_t)b * p.Hq + h) * p.nqb + qb) * p.ntk;
    if (ntk == 0) {  // workgroup uniform
      for (int j = tid; j < p.ntk; j += 256) mrow[j] = 0.f;
      return;
    }
  }
  const int q0 = qb * 128 + wave * 32;
  const int row = q0 + r;
  const int rowc = min(row, p.M - 1);
  const bool wave_live = q0 < p.M;  // wave uniform

  // Q^T fragments (B operand) and the row's scale, indexed as prepare_q of the attention kernels
  v4i qf[KS];
  float qsc;
  {
    const int8_t* qp = p.q + b * p.qsb + h * p.qsh + (int64_t)rowc * p.qsn + 16 * hh;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const v4i*>(qp + 32 * ks);
    int qi;
    if (p.qgran == SAGE_GRAN_PER_BLOCK) qi = rowc / p.blkq;
    else if (p.qgran == SAGE_GRAN_PER_WARP) qi = rowc / p.warpq;
    else qi = (rowc / p.warpq) * 8 + (rowc & 7);
    qsc = p.q_scale[((int64_t)b * p.Hq + h) * p.gq + qi] * p.logit_mult;
  }
  // K scales of tile j as load_kscales: 4 per tile (per_thread; index (key % 8) / 2 = 2 hh + ((e & 3) >> 1)) or 1
  const float* ksp = p.k_scale + ((int64_t)b * p.Hk + hk) * p.gk;
  auto tile_scales = [&](const int j, float& sc0, float& sc1) __attribute__((always_inline)) {
    if constexpr (KTHREAD) {
      const float4 kk = uniform_load4(ksp + 4 * j);
      sc0 = (hh ? kk.z : kk.x) * qsc;
      sc1 = (hh ? kk.w : kk.y) * qsc;
    } else {
      sc0 = sc1 = uniform_load1(ksp + j) * qsc;
    }
  };

  // staging: thread t owns chunks c = t + 256 i of a tile: key row c / KCH, 16-B chunk c % KCH
  const int8_t* kg = p.k + b * p.ksb + hk * p.ksh;
  int st_row[KC], st_pos[KC], st_lds[KC];
#pragma unroll
  for (int i = 0; i < KC; ++i) {
    const int c = tid + i * 256;
    st_row[i] = c / KCH; st_pos[i] = (c % KCH) * 16;
    st_lds[i] = st_row[i] * D + (((c % KCH) ^ k_swz<D>(st_row[i])) << 4);
  }
  auto load_tile = [&](const int j, v4i (&reg)[KC]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < KC; ++i)
      reg[i] = *reinterpret_cast<const v4i*>(kg + (int64_t)min(64 * j + st_row[i], nkeys - 1) * p.ksn + st_pos[i]);
  };
  auto store_tile = [&](const v4i (&reg)[KC]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < KC; ++i) *reinterpret_cast<v4i*>(k_lds + st_lds[i]) = reg[i];
  };
  int k_rd[KS];  // K A-fragment: row r (+ 32 mt), chunk 2 ks + hh
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) k_rd[ks] = r * D + (((2 * ks + hh) ^ k_swz<D>(r)) << 4);

  // base-2 logits of tile j out of the LDS image
  auto logits = [&](const int j, float (&t)[2][16]) __attribute__((always_inline)) {
    float sc0, sc1;
    tile_scales(j, sc0, sc1);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      v16i s;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = 0;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const v4i a = *reinterpret_cast<const v4i*>(k_lds + k_rd[ks] + mt * 32 * D);
        s = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, qf[ks], s, 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) t[mt][e] = (float)s[e] * ((e & 2) ? sc1 : sc0);
    }
    if (j == ntk - 1) {  // the sequence end, as mask_limit: one compare against a per-lane limit
      const int lim = nkeys - 1 - (j << 6) - 4 * hh;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          t[mt][e] = (32 * mt + (e & 3) + 8 * (e >> 2) <= lim) ? t[mt][e] : -__builtin_huge_valf();
    }
  };
  // the lane's 32 values by a pairwise tree
  auto tree32 = [&](float (&x)[2][16]) __attribute__((always_inline)) -> float {
#pragma unroll
    for (int st = 1; st < 16; st <<= 1)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 16; e += 2 * st) x[mt][e] += x[mt][e + st];
    return x[0][0] + x[1][0];
  };

  // one sweep over the key tiles: `body(j)` runs with tile j published in LDS, `between(j)` between the two barriers in
  // front of it (every wave has left tile j - 1)
  auto sweep = [&](auto&& between, auto&& body) __attribute__((always_inline)) {
    v4i reg[KC];
    load_tile(0, reg);
    for (int j = 0; j < ntk; ++j) {
      __syncthreads();
      between(j);
      store_tile(reg);
      if (j + 1 < ntk) load_tile(j + 1, reg);
      __syncthreads();
      if (wave_live) body(j);
    }
  };

  // ---- pass 1: row maximum and row sum
  float m_run = -1e30f, l_run = 0.f;  // finite start: a lane whose keys are all masked keeps l = 0 without a NaN
  sweep([](const int) {}, [&](const int j) __attribute__((always_inline)) {
    float t[2][16];
    logits(j, t);
    float mx = t[0][0];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) mx = fmaxf(mx, t[mt][e]);
    const float m_new = fmaxf(m_run, mx);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) t[mt][e] = exp2_raw(t[mt][e] - m_new);
    l_run = l_run * exp2_raw(m_run - m_new) + tree32(t);
    m_run = m_new;
  });
  float m_row, inv_l;
  {
    const float m_o = __shfl_xor(m_run, 32), l_o = __shfl_xor(l_run, 32);
    m_row = fmaxf(m_run, m_o);
    const float l_row = __fadd_rn(__fmul_rn(l_run, exp2_raw(m_run - m_row)), __fmul_rn(l_o, exp2_raw(m_o - m_row)));
    inv_l = 1.0f / l_row;  // l_row >= 1 for a live wave: the row's maximum contributes 2^0
  }

  // ---- pass 2: normalised probabilities, reduced to one number per wave and tile
  const int c_rows = min(128, p.M - qb * 128);
  auto emit = [&](const int j) __attribute__((always_inline)) {  // the entry of tile j - 1: its four numbers are in LDS
    if (tid == 0 && j > 0) mrow[j - 1] = (((wpart[0] + wpart[1]) + wpart[2]) + wpart[3]) / (float)c_rows;
  };
  if (!wave_live && lane == 0) wpart[wave] = 0.f;  // published by the first barrier of the sweep
  sweep(emit, [&](const int j) __attribute__((always_inline)) {
    float t[2][16];
    logits(j, t);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) t[mt][e] = exp2_raw(t[mt][e] - m_row) * inv_l;
    float part = tree32(t);
    part = wave_sum_fixed(row < p.M ? part : 0.f);
    if (lane == 0) wpart[wave] = part;
  });
  __syncthreads();
  emit(ntk);
  if constexpr (KVLEN)
    for (int j = ntk + tid; j < p.ntk; j += 256) mrow[j] = 0.f;  // the tiles beyond the batch's keys
}

// ------------------------------------------------------------------------------------------------
// recall of a plan
// ------------------------------------------------------------------------------------------------
struct RecallParams {
  const int* lists;
  const float* mass;
  float* recall;
  int* kept;
  int64_t rows;
  int ntk, row_ints;
  int64_t rows_b;          // KVLEN only: list rows per batch, Hq * ceil(M/128)
  const int32_t* kv_lens;  // KVLEN only (else null): int32 [B], batch b has ceil(clamp(kv_lens[b], 0, N) / 64) key tiles
};

// One wave per list row, four rows per workgroup.  The sum is taken in TILE slots, not in list positions: lane l adds, in
// ascending order, the mass of the listed tiles j with j % 64 == l (an unlisted tile adds nothing), then wave_sum_fixed.  A
// list that keeps more tiles changes no slot of the others, so every term of the tree only grows: the recall of a superset
// is not smaller, in fp32 as in exact arithmetic -- what the bisection of the tuner rests on.
// Membership without a search: the lists ascend, so the entries that fall into the 64 tiles of a step are the next ones of
// the list, at most 64: each lane holds one and raises the flag of its tile in the wave's 64 words of LDS.
// KVLEN (sage_block_plan_recall_kvlen): the batch of the row has ntk_b key tiles; the steps stop in front of ntk_b and an
// entry counts only below it, whatever `mass` holds beyond -- the same slots and the same tree as on the list and the mass cut
// to ntk_b columns.  `kept` is the number of entries that counted.  The lists are only read.
template <bool KVLEN>
__global__ __launch_bounds__(256) void plan_recall_kernel(const RecallParams p) {
  __shared__ int win[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  if (row >= p.rows) return;
  const int* lst = p.lists + row * p.row_ints;
  const int count = lst[0];
  const int cnt = min(max(count, 0), p.ntk);  // entries that are read
  const float* mrow = p.mass + row * p.ntk;
  int ntk = p.ntk;
  if constexpr (KVLEN)  // ntk_b, wave uniform
    ntk = (min(max(uniform_load_i32(p.kv_lens + ((int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(w)) / p.rows_b), 0),
               p.ntk << 6) + 63) >> 6;
  float acc = 0.f;
  int pos = 0;
  for (int j0 = 0; j0 < ntk; j0 += 64) {
    const int e = pos + lane < cnt ? lst[1 + pos + lane] : 0x7fffffff;
    const bool here = e >= j0 && e < (KVLEN ? min(j0 + 64, ntk) : j0 + 64);
    win[w][lane] = 0;
    wave_lds_fence();
    if (here) win[w][e - j0] = 1;
    wave_lds_fence();
    const int j = j0 + lane;
    if (win[w][lane] != 0 && j < ntk) acc += mrow[j];
    pos += __popcll(__ballot(here));
    // (a lane clears only the word it has just read; the other lanes write it behind the next fence)
  }
  acc = wave_sum_fixed(acc);
  if (lane == 0) {
    p.recall[row] = acc;
    p.kept[row] = KVLEN ? pos : count;
  }
}

}  // namespace sage

using namespace sage;

static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// sage_attn_tile_mass and its twin with per-batch lengths (kvlen: kv_lens is required)
static int tile_mass(const sage_tensor* q8, const sage_tensor* k8, const float* q_scale, const float* k_scale, int B, int Hq,
                     int Hk, int M, int N, int D, int qk_gran, int blkq, int warpq, float sm_scale, int logit_mult_is_one,
                     float* mass, bool kvlen, const int32_t* kv_lens, sage_stream_t stream) {
  if (kvlen && (!kv_lens || !aligned4(kv_lens))) return SAGE_ERR_INVALID_ARGUMENT;
  if (!tensor_ok(q8, 16) || !tensor_ok(k8, 16) || !q_scale || !k_scale || !mass) return SAGE_ERR_INVALID_ARGUMENT;
  if (!aligned4(q_scale) || !aligned4(k_scale) || !aligned4(mass)) return SAGE_ERR_INVALID_ARGUMENT;
  if (B <= 0 || Hq <= 0 || Hk <= 0 || M <= 0 || N <= 0 || Hq % Hk != 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (!logit_mult_is_one && !(sm_scale > 0.f && sm_scale < 1.0e30f)) return SAGE_ERR_INVALID_ARGUMENT;
  if (D != 64 && D != 128) return SAGE_ERR_UNSUPPORTED_HEAD_DIM;
  if (qk_gran == SAGE_GRAN_PER_BLOCK) return SAGE_ERR_UNSUPPORTED;  // the block-sparse operators do not take it either
  if (qk_gran != SAGE_GRAN_PER_WARP && qk_gran != SAGE_GRAN_PER_THREAD) return SAGE_ERR_INVALID_ARGUMENT;
  if (blkq != 64 && blkq != 128) return SAGE_ERR_INVALID_ARGUMENT;
  if ((warpq != 16 && warpq != 32 && warpq != 64 && warpq != 128) || blkq % warpq != 0) return SAGE_ERR_INVALID_ARGUMENT;
  const bool kthread = qk_gran == SAGE_GRAN_PER_THREAD;
  if (kthread && !aligned16(k_scale)) return SAGE_ERR_INVALID_ARGUMENT;  // four scales of a tile in one 16-byte load
  MassParams p;
  p.q = (const int8_t*)q8->data; p.qsb = q8->stride_b; p.qsh = q8->stride_h; p.qsn = q8->stride_n;
  p.k = (const int8_t*)k8->data; p.ksb = k8->stride_b; p.ksh = k8->stride_h; p.ksn = k8->stride_n;
  p.q_scale = q_scale; p.k_scale = k_scale; p.mass = mass;
  p.Hq = Hq; p.Hk = Hk; p.M = M; p.N = N;
  p.nqb = (int)(((int64_t)M + 127) / 128); p.ntk = (int)(((int64_t)N + 63) / 64);
  const int nblkq = (int)(((int64_t)M + blkq - 1) / blkq);
  p.gq = kthread ? nblkq * (blkq / warpq) * 8 : nblkq * (blkq / warpq);
  p.gk = kthread ? p.ntk * 4 : p.ntk;
  p.qgran = qk_gran; p.blkq = blkq; p.warpq = warpq;
  p.logit_mult = logit_mult_is_one ? 1.0f : sm_scale * kLog2e;
  p.B = B; p.kv_lens = kv_lens;
  // (Q and K are addressed with 64-bit offsets, not through buffer descriptors: no 2 GiB slice window)
  const int64_t grid = (int64_t)B * Hq * p.nqb;
  if (grid >= ((int64_t)1 << 31)) return SAGE_ERR_TOO_LARGE;
  launch_begin();
  by_dim(D, [&](auto d) {
    by_flag(kthread, [&](auto kt) {
      by_flag(kvlen, [&](auto len) {
        hipLaunchKernelGGL((tile_mass_kernel<decltype(d)::value, decltype(kt)::value, decltype(len)::value>),
                           dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p);
      });
    });
  });
  return launch_status();
}

extern "C" int sage_attn_tile_mass(const sage_tensor* q8, const sage_tensor* k8, const float* q_scale, const float* k_scale,
                                   int B, int Hq, int Hk, int M, int N, int D, int qk_gran, int blkq, int warpq,
                                   float sm_scale, int logit_mult_is_one, float* mass, sage_stream_t stream) {
  return tile_mass(q8, k8, q_scale, k_scale, B, Hq, Hk, M, N, D, qk_gran, blkq, warpq, sm_scale, logit_mult_is_one, mass, false,
                   nullptr, stream);
}

extern "C" int sage_attn_tile_mass_kvlen(const sage_tensor* q8, const sage_tensor* k8, const float* q_scale,
                                         const float* k_scale, int B, int Hq, int Hk, int M, int N, int D, int qk_gran,
                                         int blkq, int warpq, float sm_scale, int logit_mult_is_one, float* mass,
                                         const int32_t* kv_lens, sage_stream_t stream) {
  return tile_mass(q8, k8, q_scale, k_scale, B, Hq, Hk, M, N, D, qk_gran, blkq, warpq, sm_scale, logit_mult_is_one, mass, true,
                   kv_lens, stream);
}

// sage_block_plan_recall and its twin with per-batch lengths (kvlen: kv_lens is required)
static int plan_recall(const int32_t* block_lists, int64_t block_lists_bytes, const float* mass, int B, int Hq, int M, int N,
                       float* recall, int32_t* kept, bool kvlen, const int32_t* kv_lens, sage_stream_t stream) {
  if (kvlen && (!kv_lens || !aligned4(kv_lens))) return SAGE_ERR_INVALID_ARGUMENT;
  if (!block_lists || !aligned16(block_lists) || !mass || !recall || !kept) return SAGE_ERR_INVALID_ARGUMENT;
  if (!aligned4(mass) || !aligned4(recall) || !aligned4(kept)) return SAGE_ERR_INVALID_ARGUMENT;
  if (B <= 0 || Hq <= 0 || M <= 0 || N <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (block_lists_bytes < block_sparse_bytes(B, Hq, M, N)) return SAGE_ERR_INVALID_ARGUMENT;
  RecallParams p;
  p.lists = (const int*)block_lists; p.mass = mass; p.recall = recall; p.kept = (int*)kept;
  p.ntk = (int)(((int64_t)N + 63) / 64); p.row_ints = (int)block_list_row(N);
  p.rows_b = (int64_t)Hq * (((int64_t)M + 127) / 128);
  p.rows = (int64_t)B * p.rows_b;
  p.kv_lens = kv_lens;
  if ((p.rows + 3) / 4 >= ((int64_t)1 << 31)) return SAGE_ERR_TOO_LARGE;
  launch_begin();
  by_flag(kvlen, [&](auto len) {
    hipLaunchKernelGGL(plan_recall_kernel<decltype(len)::value>, dim3((unsigned)((p.rows + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, p);
  });
  return launch_status();
}

extern "C" int sage_block_plan_recall(const int32_t* block_lists, int64_t block_lists_bytes, const float* mass, int B, int Hq,
                                      int M, int N, float* recall, int32_t* kept, sage_stream_t stream) {
  return plan_recall(block_lists, block_lists_bytes, mass, B, Hq, M, N, recall, kept, false, nullptr, stream);
}

extern "C" int sage_block_plan_recall_kvlen(const int32_t* block_lists, int64_t block_lists_bytes, const float* mass, int B,
                                            int Hq, int M, int N, float* recall, int32_t* kept, const int32_t* kv_lens,
                                            sage_stream_t stream) {
  return plan_recall(block_lists, block_lists_bytes, mass, B, Hq, M, N, recall, kept, true, kv_lens, stream);
}
