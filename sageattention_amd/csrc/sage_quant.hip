// Pre-pass kernels of the SageAttention hot path for gfx950 (every one a single pass over its tensor):
//   K0  k_mean            (replaces torch k.mean at sageattention/core.py:612)
//   K1  quant_qk_int8     (replaces QuantInt8Kernel csrc/fused/fused.cu:64-198 and the Triton
//                          quantizers sageattention/triton/quant_per_{block,thread}.py)
//                         one block per workgroup (quant_qk_int8_kernel) or, for dense K, several consecutive blocks of a
//                         head per workgroup with the next block's rows prefetched (k_quant_stream_kernel); with the FP8 V
//                         quantizer in one launch: kv_quant_kernel / kv_quant_stream_kernel
//   K2  sub_mean_f16      (replaces SubMeanKernel csrc/fused/fused.cu:200-260)
// Algorithmic traffic per element: 2 B read + 1 B written (K1), 2 B read (K0); every thread moves 16 B per load (8
// fp16/bf16), the widest coalesced access on CDNA4.  The floor of each kernel is that traffic over the streaming rate of
// HBM (6.29 TB/s measured), but a quantizer reaches it only while its vector work stays small: at (4,32,8192,128) every
// vector instruction per element is 3.4-3.9 us of issue time on the whole chip (134 M elements over 1024 SIMDs x 16 lanes
// at 2.1-2.4 GHz) against a floor of 64 us, with four or five waves per SIMD and a barrier per block to hide it behind.
// The streaming K quantizer held 27 vector instructions per element outside its exact-division fallback and took 98 us
// there -- co-limited by vector issue, not by HBM; written for what a dense K call fixes it holds 9 and takes 66 us
// (profiles/k_quant_valu_diet.md: the instruction census and the in-step traces).
// Compiled with -ffp-contract=off: the integer outputs must match the oracle bit for bit.
#include <algorithm>
#include <climits>
#include "../../include/sageattn_hip_kvcache.h"
#include "../../include/sageattn_hip_paged.h"
#include "../../include/sageattn_hip_paged_rows.h"
#include "sage_entry.h"
#include "sage_fp8_kernels.h"

namespace sage {

// ------------------------------------------------------------------------------------------------
// K0: k_mean, deterministic two-pass reduction
// ------------------------------------------------------------------------------------------------
constexpr int KMEAN_ROWS = 256;  // granule of the pass-1 chunks (rows)
// Rows per pass-1 chunk: a multiple of KMEAN_ROWS chosen so that a sequence never has more than 16 chunks -- the quantizers
// then ALWAYS finish the statistics themselves (16 partial rows per head out of L2), i.e. the K pre-pass is two launches
// and the FP8 operator's K + V pre-pass is two launches at every length (up to 4096 rows the chunks are KMEAN_ROWS rows;
// beyond, the partial sums are taken over longer chunks).
__host__ __device__ __forceinline__ int kmean_chunk_rows(int N) {
  const int c256 = (N + KMEAN_ROWS - 1) / KMEAN_ROWS;
  return KMEAN_ROWS * ((c256 + 15) / 16 > 0 ? (c256 + 15) / 16 : 1);
}

// chunks of pass 1 (kmean_chunk_rows): at most 16
__host__ __device__ __forceinline__ int kmean_chunks(int N) {
  const int rows = kmean_chunk_rows(N);
  return (N + rows - 1) / rows;
}
// Per-batch key lengths (the _kvlen entry points): batch b has the rows [0, len_b), len_b = clamp(kv_lens[b], 0, N), and is
// chunked as a call on len_b rows would be.  The most chunks a batch of up to N rows can have (a shorter batch may have MORE
// chunks than one of N rows -- 4096 rows are 16 chunks of 256, 4400 rows 9 of 512): the chunk slots per head of the workspace
__host__ __device__ __forceinline__ int kmean_max_chunks(int N) {
  const int c256 = (N + KMEAN_ROWS - 1) / KMEAN_ROWS;
  return c256 < 16 ? c256 : 16;
}
// kv_lens as the last argument of a pre-pass kernel: the pointer in its KVLEN instantiation, in the other an empty struct.
// (A pointer that is merely not read moves the hidden arguments behind it -- the grid size -- by 8 bytes; the one byte of
// the empty struct goes into the padding behind the int that every one of these kernels has in front of it, and the
// instantiations without lengths keep their instruction streams: profiles/prepass_one_text.md.)
template <bool KVLEN>
struct KvLens {
  KvLens(const int32_t*) {}
};
template <>
struct KvLens<true> {
  const int32_t* p;
  KvLens(const int32_t* kv_lens) : p(kv_lens) {}
};
__device__ __forceinline__ int kv_len_of(const int32_t* __restrict__ kv_lens, int b, int N) { return min(max(kv_lens[b], 0), N); }

// chunk s (KMEAN_ROWS rows) of head (b, h) of H: column sums -> part[b][h][s][D]; `red`: 256/(D/8) x (D+1) floats of LDS
template <int D, bool BF16>
__device__ __forceinline__ void k_mean_partial_body(const uint16_t* __restrict__ k, int64_t sb, int64_t sh, int64_t sn, int N,
                                                    float* __restrict__ part, int S, int s, int h, int b, int H,
                                                    float (*red)[D + 1]) {
  constexpr int TPR = D / 8;       // threads per row
  constexpr int RPP = 256 / TPR;   // rows per pass
  const int tr = threadIdx.x / TPR, tc = threadIdx.x % TPR;
  const uint16_t* base = k + b * sb + h * sh + tc * 8;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int rows = kmean_chunk_rows(N);
  const int r0 = s * rows;
  // Whole chunks (all but the last of a sequence) take the loop without a row test: hipcc sinks a conditional load into
  // its branch and then waits for every load before it issues the next one (one 16-B load in flight per thread: the kernel
  // ran at the latency of sixteen dependent round trips); unconditional, the unrolled loop keeps eight in flight.  Same
  // additions in the same order.
  if (r0 + rows <= N) {
#pragma unroll 8
    for (int i = 0; i < rows / RPP; ++i) {
      const uint4 u = *reinterpret_cast<const uint4*>(base + (int64_t)(r0 + i * RPP + tr) * sn);
      float f[8];
      unpack8<BF16>(u, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
  } else {
#pragma unroll 4
    for (int i = 0; i < rows / RPP; ++i) {
      const int row = r0 + i * RPP + tr;
      if (row < N) {
        const uint4 u = *reinterpret_cast<const uint4*>(base + (int64_t)row * sn);
        float f[8];
        unpack8<BF16>(u, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[tr][tc * 8 + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < D) {
    float sum = 0.f;
    for (int r = 0; r < RPP; ++r) sum += red[r][threadIdx.x];  // fixed order
    part[(((int64_t)b * H + h) * S + s) * D + threadIdx.x] = sum;
  }
}

// KVLEN (per-batch key lengths): the chunks of batch b are those of a call on its len_b rows,
// in the S chunk slots of its heads; the grid is sized for S slots, and the workgroups of chunks a batch does not have
// leave before any barrier
template <int D, bool BF16, bool KVLEN>
__global__ __launch_bounds__(256) void k_mean_partial_kernel(const uint16_t* __restrict__ k, int64_t sb, int64_t sh,
                                                             int64_t sn, int N, float* __restrict__ part, int S,
                                                             const KvLens<KVLEN> kv_lens) {
  __shared__ float red[256 / (D / 8)][D + 1];
  if constexpr (KVLEN) {
    N = kv_len_of(kv_lens.p, blockIdx.z, N);
    if ((int)blockIdx.x >= kmean_chunks(N)) return;  // (an empty batch has none)
  }
  k_mean_partial_body<D, BF16>(k, sb, sh, sn, N, part, S, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.y, red);
}

template <bool BF16>
__global__ void k_mean_final_kernel(const float* __restrict__ part, int S, int D, int N, uint16_t* __restrict__ km) {
  const int64_t bh = blockIdx.x;
  const int d = threadIdx.x;
  if (d >= D) return;
  float sum = 0.f;
  for (int s0 = 0; s0 < S; s0 += 8) {  // 8 partials in flight, added in chunk order
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(bh * S + min(s0 + u, S - 1)) * D + d];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (s0 + u < S) sum += v[u];
  }
  km[bh * D + d] = f32_to_elem_bits<BF16>(sum / (float)N);
}

// ------------------------------------------------------------------------------------------------
// K1: INT8 quantizer, all granularities
// ------------------------------------------------------------------------------------------------
// (QuantParams, the kernels' parameter block: sage_entry.h)

// max over the TPR (8 or 16) consecutive lanes that hold one row, on DPP (quad swaps, then the mirrored half rows / rows): every
// lane ends with the row's maximum; 3-4 DPP maxima instead of as many ds_bpermute round trips.  The values are finite and
// non-negative (maxima of |x| that start at 0), so their bit patterns order like the numbers and the maximum is taken on
// the bits: an integer maximum needs no canonicalising v_max x, x in front, and with every lane a valid source (full row
// and bank masks, permutations only) the lane move folds into the v_max_u32 as its DPP operand -- ONE instruction per
// step where fmaxf(a, moved a) cost four (v_mov 0, v_mov_b32_dpp, v_max a, a, v_max).  (A maximum does not depend on the
// order it is taken in: bit-identical to the xor butterfly.)
template <int CTRL>
__device__ __forceinline__ unsigned int dpp_max_u32(unsigned int x) {
  return max(x, (unsigned int)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, 0xf, 0xf, true));
}
template <int TPR>
__device__ __forceinline__ float row_lanes_max(float a) {
  static_assert(TPR == 8 || TPR == 16, "a row is 8 or 16 lanes");
  unsigned int u = __float_as_uint(a);
  u = dpp_max_u32<0xB1>(u);    // quad_perm [1,0,3,2]
  u = dpp_max_u32<0x4E>(u);    // quad_perm [2,3,0,1]
  u = dpp_max_u32<0x141>(u);   // row_half_mirror: the other quad of the 8 lanes
  if constexpr (TPR == 16) u = dpp_max_u32<0x140>(u);  // row_mirror: the other half of the 16 lanes
  return __uint_as_float(u);
}

__device__ __forceinline__ int group_of_row(int lr, int gran, int is_key, int warp_shift) {
  // group-id maps: per_block: all rows of the workgroup; per_warp: lr/warp; per_thread:
  // triton/quant_per_thread.py:27-36 (Q: r%8) and :73-80 (K: (r%8)/2).
  if (gran == SAGE_GRAN_PER_BLOCK) return 0;
  const int w = lr >> warp_shift;
  if (gran == SAGE_GRAN_PER_WARP) return w;
  return is_key ? w * 4 + ((lr & 7) >> 1) : w * 8 + (lr & 7);
}

// ---- the quantizer in three steps (the streaming K quantizer below shares the geometry, the mean and sub_mean8) ----
template <int D, int BLK>
struct QuantGeom {
  static constexpr int TPR = D / 8;        // threads per row (16 B each)
  static constexpr int RPP = 256 / TPR;    // rows per pass of the workgroup
  static constexpr int NP = BLK / RPP;     // passes per block = 16-B loads per thread
  static_assert(NP >= 1, "block too small");
};

// step 1: the rows of block `blk` (rows past the end read as zeros).  xbase: head base + this thread's column offset
template <int D, int BLK>
__device__ __forceinline__ void quant_load_rows(const uint16_t* xbase, const int64_t xsn, const int blk, const int N_,
                                                uint4 (&raw)[QuantGeom<D, BLK>::NP]) {
  using G = QuantGeom<D, BLK>;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // see quant_block
  const int tr = tid / G::TPR;
#pragma unroll
  for (int i = 0; i < G::NP; ++i) {
    const int row = blk * BLK + i * G::RPP + tr;
    raw[i] = make_uint4(0, 0, 0, 0);
    if (row < N_) raw[i] = *reinterpret_cast<const uint4*>(xbase + (int64_t)row * xsn);
  }
}

// step 2 (once per head): the mean as 8 storage-dtype values per thread column.  Holds the workgroup's FIRST barrier (which
// also publishes the zeroed group maxima) and, in the mean_part form, a second one.  mpart: 16 x D floats (16-byte aligned)
template <int D, bool BF16>
__device__ __forceinline__ uint4 quant_mean_bits(const QuantParams& p, const int h, const int b, const int H, const bool store_km,
                                                 float (*mpart)[D]) {
  constexpr int TPR = D / 8;
  const int tr = threadIdx.x / TPR, tc = threadIdx.x % TPR;
  // mean_part: thread row s fetches chunk s (ONE round trip to L2 for all S chunks instead of S dependent ones: at 2048
  // rows the quantizer spent more time on these than on its block), LDS hands the first thread row all chunks
  if (p.mean_part && tr < p.S) {
    const float* pp = p.mean_part + (((int64_t)b * H + h) * p.S + tr) * D + tc * 8;
    *reinterpret_cast<float4*>(&mpart[tr][tc * 8]) = *reinterpret_cast<const float4*>(pp);
    *reinterpret_cast<float4*>(&mpart[tr][tc * 8 + 4]) = *reinterpret_cast<const float4*>(pp + 4);
  }
  __syncthreads();  // gmax zeroed, mpart filled
  // mean_part form: the FIRST thread row finishes the reduction (chunk order, as k_mean_final_kernel; an IEEE division per
  // column) and hands the bits to the other rows through LDS -- every thread doing it for itself cost 8 divisions + 8 S
  // adds per thread, a fifth of the kernel's vector work, and the rows of the block are still on their way from HBM.
  uint4 mbits = make_uint4(0u, 0u, 0u, 0u);
  if (p.mean_part) {
    if (tr == 0) {
      float sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int s_ = 0; s_ < p.S; ++s_) {
        const float4 a = *reinterpret_cast<const float4*>(&mpart[s_][tc * 8]), c = *reinterpret_cast<const float4*>(&mpart[s_][tc * 8 + 4]);
        sum[0] += a.x; sum[1] += a.y; sum[2] += a.z; sum[3] += a.w; sum[4] += c.x; sum[5] += c.y; sum[6] += c.z; sum[7] += c.w;
      }
      uint32_t w[4];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint16_t bits = f32_to_elem_bits<BF16>(sum[j] / (float)p.N);
        if (j & 1) w[j >> 1] |= (uint32_t)bits << 16; else w[j >> 1] = bits;
      }
      mbits = make_uint4(w[0], w[1], w[2], w[3]);
      // (this thread alone read columns tc*8 .. tc*8+7 of mpart, so it may overwrite them in row 0)
      *reinterpret_cast<uint4*>(&mpart[0][tc * 8]) = mbits;
      if (store_km) *reinterpret_cast<uint4*>(p.km_out + ((int64_t)b * H + h) * D + tc * 8) = mbits;
    }
    __syncthreads();
    mbits = *reinterpret_cast<const uint4*>(&mpart[0][tc * 8]);
  } else if (p.mean) {
    // packed sequences share one mean over all tokens ([1,H,D], core.py:461)
    mbits = *reinterpret_cast<const uint4*>(p.mean + ((int64_t)(p.cu ? 0 : b) * H + h) * D + tc * 8);
  }
  return mbits;
}

// x - mean for the 8 elements of one 16-byte load (no mean: mbits = 0 and x - 0 is x in either form).
//   TRITON: `k - km` in the input dtype (torch).   CUDA: in fp32 (fused.cu).
// fp16, TRITON: the subtraction runs as v_pk_add_f16 -- the correctly rounded fp16 difference, which is what rounding the
// fp32 difference of two fp16 values gives as well (24 >= 2*11+2 bits: the double rounding is innocuous) -- 4 packed
// subtractions + 8 converts per 8 elements instead of 8 + 8 + 16.  mean_f: the mean unpacked (read unless TRITON && !BF16)
template <bool BF16, bool TRITON>
__device__ __forceinline__ void sub_mean8(const uint4& raw, const uint4& mbits, const float (&mean_f)[8], float (&xf)[8]) {
  if constexpr (TRITON && !BF16) {
    const uint32_t xw[4] = {raw.x, raw.y, raw.z, raw.w}, mw[4] = {mbits.x, mbits.y, mbits.z, mbits.w};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const v2h d = __builtin_bit_cast(v2h, xw[w]) - __builtin_bit_cast(v2h, mw[w]);
      xf[2 * w] = (float)d[0];
      xf[2 * w + 1] = (float)d[1];
    }
  } else {
    unpack8<BF16>(raw, xf);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xf[j] = xf[j] - mean_f[j];
      if constexpr (TRITON) xf[j] = round_to_elem<BF16>(xf[j]);
    }
  }
}

// step 3: block `blk` from its rows: group maxima (gmax: 64 zeroed dwords), ONE barrier, scales, rounding, stores.
template <int D, int BLK, bool BF16, bool TRITON>
__device__ __forceinline__ void quant_block(const QuantParams& p, const int blk, const int h, const int b, const int H, const int N_,
                                            const int64_t o_boff, uint4 (&raw)[QuantGeom<D, BLK>::NP], const uint4 mbits,
                                            unsigned int* gmax) {
  using G = QuantGeom<D, BLK>;
  constexpr int TPR = G::TPR, RPP = G::RPP, NP = G::NP;
  // (the thread id is made opaque: hipcc otherwise computes every row / group / address term that depends only on it up
  //  front and keeps it alive across the barrier -- several instantiations then lose a wave per SIMD to the registers)
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int tr = tid / TPR, tc = tid % TPR;
  float xf[NP][8];
  float dvec[8];
  if (p.dot_vec) {
    const int Hk = H / p.dot_group;
    const uint4 ud = *reinterpret_cast<const uint4*>(p.dot_vec + ((int64_t)b * Hk + h / p.dot_group) * D + tc * 8);
    unpack8<BF16>(ud, dvec);
  }

  // x - mean (sub_mean8), times the multiplier, and the group maxima
  {
    float mean_f[8];
    if constexpr (!TRITON || BF16) unpack8<BF16>(mbits, mean_f);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int lr = i * RPP + tr;
      const int row = blk * BLK + lr;
      const bool valid = row < N_;
      if (p.dot_vec) {
        float xr[8];
        unpack8<BF16>(raw[i], xr);
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += xr[j] * dvec[j];
#pragma unroll
        for (int o = 1; o < TPR; o <<= 1) dot += __shfl_xor(dot, o);
        if (tc == 0 && valid) p.dot_out[((int64_t)b * H + h) * p.N + row] = dot;
      }
      sub_mean8<BF16, TRITON>(raw[i], mbits, mean_f, xf[i]);
      float amax = 0.f;
      const float mult_row = valid ? p.mult : 0.f;  // rows past the end contribute zeros (finite inputs: raw is 0 there)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xf[i][j] = xf[i][j] * mult_row;
        amax = fmaxf(amax, fabsf(xf[i][j]));
      }
      amax = row_lanes_max<TPR>(amax);
      if (tc == 0) atomicMax(&gmax[group_of_row(lr, p.gran, p.is_key, p.warp_shift)], __float_as_uint(amax));
    }
  }
  __syncthreads();

  const int groups_per_blk = p.gran == SAGE_GRAN_PER_BLOCK ? 1
                             : p.gran == SAGE_GRAN_PER_WARP ? BLK >> p.warp_shift
                                                            : (BLK >> p.warp_shift) * (p.is_key ? 4 : 8);
  const float eps = (p.gran == SAGE_GRAN_PER_THREAD) ? 0.0000001f : 0.f;
  if (threadIdx.x < groups_per_blk) {
    const float a = __uint_as_float(gmax[threadIdx.x]);
    const float sc = TRITON ? a / 127.f + eps : fmaxf(a, 0.0000001f) / 127.f;
    p.scale[b * p.ss_b + h * p.ss_h + blk * p.ss_blk + threadIdx.x] = sc;
  }

  int8_t* obase = p.out + o_boff + h * p.osh + blk * p.o_blk + tc * 8;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int lr = i * RPP + tr;
    const int row = blk * BLK + lr;
    const float a = __uint_as_float(gmax[group_of_row(lr, p.gran, p.is_key, p.warp_shift)]);
    int q[8];
    // No clamp on the two fast paths: |x| <= a (a is the maximum of a group x belongs to), so |x * r| <= 127 (1 + 3 ulp)
    // and rint() of it is at most 127 in magnitude.
    if constexpr (TRITON) {
      // q = trunc(x/sc + 0.5*sign) with an IEEE division (quant_per_block.py:42-44).  The division costs ~10 VALU
      // ops per element and made the kernel VALU-bound, so: multiply by the correctly rounded reciprocal
      // (|x*r - x/sc| <= 1.5 ulp <= 2.3e-5 for |x/sc| <= 127, plus <= 7.6e-6 from the +0.5) and fall back to the exact
      // division, for the whole 8-element chunk of the wave, only when some value lands within 2^-14 of a
      // rounding boundary, where the two could differ (~6 % of the chunks).  Bit-exact by construction.
      const float sc = a / 127.f + eps;
      const float r = 1.0f / sc;
      bool near = false;
#pragma unroll
      for (int j = 0; j < 8; ++j) q[j] = round_half_away_fast(xf[i][j] * r, near);
      if (__builtin_amdgcn_ballot_w64(near || !(fabsf(r) < 3.0e38f)) != 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float y = xf[i][j] / sc;  // IEEE division
          y = y + (y >= 0.f ? 0.5f : -0.5f);
          q[j] = min(max((int)y, -128), 127);  // truncation, as tl `.to(int8)`
        }
      }
    } else {
      const float inv = 127.f / fmaxf(a, 0.0000001f);
#pragma unroll
      for (int j = 0; j < 8; ++j) q[j] = (int)rintf(xf[i][j] * inv);  // cvt.rni (fused.cu:176-181)
    }
    const uint32_t w0 = pack_i8x4(q[0], q[1], q[2], q[3]), w1 = pack_i8x4(q[4], q[5], q[6], q[7]);
    if (row < N_) *reinterpret_cast<uint2*>(obase + (int64_t)lr * p.osn) = make_uint2(w0, w1);
  }
}

// block `blk` (BLK rows) of head (b, h) of H.  LDS: gmax = 64 dwords, mpart = 16 x D floats (16-byte aligned)
template <int D, int BLK, bool BF16, bool TRITON>
__device__ __forceinline__ void quant_qk_int8_body(const QuantParams& p, const int blk, const int h, const int b, const int H,
                                                   unsigned int* gmax, float (*mpart)[D]) {
  int N_ = p.N;
  int64_t x_boff = b * p.xsb, o_boff = b * p.osb;
  if (p.cu) {
    const int lo = p.cu[b];
    N_ = p.cu[b + 1] - lo;
    if (blk * BLK >= N_) return;  // uniform for the workgroup
    x_boff = (int64_t)lo * p.xsn;
    o_boff = (int64_t)lo * p.osn;
  }
  if (threadIdx.x < 64) gmax[threadIdx.x] = 0u;
  // the block's rows first: everything below overlaps with this one trip to HBM
  uint4 raw[QuantGeom<D, BLK>::NP];
  quant_load_rows<D, BLK>(p.x + x_boff + h * p.xsh + (threadIdx.x % (D / 8)) * 8, p.xsn, blk, N_, raw);
  const uint4 mbits = quant_mean_bits<D, BF16>(p, h, b, H, blk == 0, mpart);
  quant_block<D, BLK, BF16, TRITON>(p, blk, h, b, H, N_, o_boff, raw, mbits, gmax);
}

// (the rounding flavour is a template parameter: with both flavours in one kernel the register allocation of the shared
//  part suffered -- 80 instead of 65 registers at head_dim 128 -- and every element paid a uniform branch)
template <int D, int BLK, bool BF16, bool TRITON>
__global__ __launch_bounds__(256, BLK * D <= 64 * 128 ? 7 : 4) void quant_qk_int8_kernel(const QuantParams p) {
  __shared__ unsigned int gmax[64];
  __shared__ __attribute__((aligned(16))) float mpart[16][D];  // chunk sums of the mean (mean_part form: S <= 16 <= RPP)
  quant_qk_int8_body<D, BLK, BF16, TRITON>(p, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.y, gmax, mpart);
}

// Streaming K quantizer (dense K, 64-row blocks): a workgroup walks `per_wg` consecutive blocks of ONE head and loads the
// rows of block i+1 before it works on block i.  With one block per workgroup a launch is one (or two) generations of
// workgroups that all sit in the same phase -- every load of the tensor issued at once, then every store -- and the
// latency chain load -> maxima -> barrier -> rounding -> store is paid once per generation with nothing beside it; here
// the next block's rows fly during the second half of the chain, stores and loads of neighbouring blocks overlap, and the
// mean of the head is finished once per workgroup instead of once per block.  Same arithmetic per block: bit-identical.
// One barrier per block: the group maxima rotate through three buffers (block i accumulates into buffer i % 3 and, behind
// its barrier, zeroes buffer (i + 2) % 3 -- last read by block i-1, whose readers have all passed this barrier, and next
// written by block i+2, behind the barrier of block i+1).
//
// The kernel is limited by vector issue as much as by HBM (profiles/k_quant_valu_diet.md), so its block is written for
// what a dense K call fixes -- is_key, 64-row blocks in one warp group, no dot_vec, mult == 1 (x * 1 is x: the multiply
// is gone), granularity per_block or per_thread as a template flag -- instead of going through quant_block:
//  * a thread's rows 16 i + tr (head_dim 128) or 32 i + tr (64) all fall into ONE group, (tr & 7) >> 1 or 0: one maximum
//    over all its elements, one DPP reduction and one LDS atomic per block instead of one per pass, and the scale, its two
//    IEEE divisions included, once per block.  (A maximum does not depend on the order: the same bits.)
//  * RAGGED (the last block of a head when N % 64 != 0) alone knows rows past the end: they are loaded as copies of row
//    N - 1, kept out of the maxima (after the subtraction they are not zeros) and not stored.  Full blocks carry no selects.

// the rows of block `blk`; CLAMP: rows past the end read row N - 1 (always in bounds; the caller ignores them)
template <int D, bool CLAMP>
__device__ __forceinline__ void k_load_rows(const uint16_t* xbase, const int64_t xsn, const int blk, const int N,
                                            uint4 (&raw)[QuantGeom<D, 64>::NP]) {
  using G = QuantGeom<D, 64>;
  const int row0 = blk * 64 + (int)threadIdx.x / G::TPR;
#pragma unroll
  for (int i = 0; i < G::NP; ++i) {
    const int row = CLAMP ? min(row0 + i * G::RPP, N - 1) : row0 + i * G::RPP;
    raw[i] = *reinterpret_cast<const uint4*>(xbase + (int64_t)row * xsn);
  }
}

// Eight quotients x / sc rounded half away from zero (the Triton quantizers, quant_per_block.py:42-44: an IEEE division,
// + 0.5 sign, truncation) as two dwords of int8, WITHOUT the division; `near` is set when the chunk must be redone with
// it.  With r = fl(1 / sc) and M = 1.5 * 2^23, per element
//     t = fma(x, r, M)      res = fma(x, r, -(t - M))
// |x r| <= 127 (1 + 2^-22) (x belongs to the group whose maximum made sc), so x r + M lies in [2^23, 2^24), where floats are
// the integers: the one rounding of the fma makes t = M + n exactly, n the integer nearest to the EXACT product x r, and
// the low byte of t's bit pattern, 0x4B400000 + n, is n as a two's-complement int8.  t - M = n is exact and res is
// x r - n to within 2^-25.  The chunk passes when every |res| <= 1/2 - 2^-14.  Then, with e = x / sc exact:
// |x r - e| <= 2^-24 |e| < 7.7e-6 (r is correctly rounded), so |e - n| < 1/2 - 5.3e-5; the reference's quotient fl(e) is within
// 7.7e-6 of e and its fl(. +- 0.5) within another 3.9e-6 (half an ulp below 128): the sum lies strictly between n and n + sign
// and truncates to n.  No clamp: |n| <= 127.  The margin in use, 1.9e-5 of 6.1e-5, leaves the 2^-14 of the contract whole.
// 3 VALU per element and 1/2 for the test (v_max3 over |res|) against mul, rndne, sub, cmp, cvt and a scalar or; the bytes
// are picked straight out of t: 3 v_perm_b32 per dword, no conversion to integer, no 16-bit shifts.
__device__ __forceinline__ uint2 round_half_away_pack8(const float (&x)[8], const float r, bool& near) {
  constexpr float M = 12582912.f;
  uint32_t tb[8];
  float res[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t = __builtin_fmaf(x[j], r, M);
    res[j] = __builtin_fmaf(x[j], r, -(t - M));
    tb[j] = __float_as_uint(t);
  }
  float m = fmaxf(fmaxf(fabsf(res[0]), fabsf(res[1])), fabsf(res[2]));
  m = fmaxf(fmaxf(m, fabsf(res[3])), fabsf(res[4]));
  m = fmaxf(fmaxf(m, fabsf(res[5])), fabsf(res[6]));
  m = fmaxf(m, fabsf(res[7]));
  near = !(m <= 0.5f - 6.1035156e-5f);  // (a NaN is near)
  return make_uint2(pack_i8x4(tb[0], tb[1], tb[2], tb[3]), pack_i8x4(tb[4], tb[5], tb[6], tb[7]));
}

// block `blk` of head (b, h) from its rows: as quant_block, for the fixed K form above.  gmax, zero_next: PER_THREAD ? 4 : 1
// group maxima of this block / of the block after next; after_phase1(): `raw` may be reloaded
template <int D, bool BF16, bool TRITON, bool PER_THREAD, bool RAGGED, typename AfterPhase1>
__device__ __forceinline__ void k_quant_block(const QuantParams& p, const int blk, const int h, const int b,
                                              uint4 (&raw)[QuantGeom<D, 64>::NP], const uint4 mbits, unsigned int* gmax,
                                              unsigned int* zero_next, AfterPhase1 after_phase1) {
  using G = QuantGeom<D, 64>;
  constexpr int TPR = G::TPR, RPP = G::RPP, NP = G::NP, NG = PER_THREAD ? 4 : 1;
  static_assert(RPP % 8 == 0, "the group of a row must not depend on the pass");
  const int tr = (int)threadIdx.x / TPR, tc = (int)threadIdx.x % TPR;
  const int g = PER_THREAD ? (tr & 7) >> 1 : 0;  // triton/quant_per_thread.py:73-80 (K: (r % 8) / 2), one warp group
  const int row0 = blk * 64 + tr;
  float xf[NP][8];
  {
    float mean_f[8];
    if constexpr (!TRITON || BF16) unpack8<BF16>(mbits, mean_f);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      sub_mean8<BF16, TRITON>(raw[i], mbits, mean_f, xf[i]);
      float am = RAGGED ? 0.f : amax;
#pragma unroll
      for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(xf[i][j]));
      if constexpr (RAGGED) amax = fmaxf(amax, row0 + i * RPP < p.N ? am : 0.f);
      else amax = am;
    }
    amax = row_lanes_max<TPR>(amax);
    if (tc == 0) atomicMax(&gmax[g], __float_as_uint(amax));
  }
  after_phase1();
  __syncthreads();
  if (threadIdx.x < NG) zero_next[threadIdx.x] = 0u;

  const float a = __uint_as_float(gmax[g]);
  // TRITON: sc = a / 127 (+ 1e-7 per_thread) and q = x / sc half away from zero;  CUDA: sc = max(a, 1e-7) / 127 and
  // q = rint(x * (127 / max(a, 1e-7))) (fused.cu:176-181).  One thread per group stores the scale (rows 0, 2, 4, 6).
  const float sc = TRITON ? a / 127.f + (PER_THREAD ? 0.0000001f : 0.f) : 0.f;
  const float r = TRITON ? 1.0f / sc : 127.f / fmaxf(a, 0.0000001f);
  if (tc == 0 && tr < 2 * NG && !(tr & 1))
    p.scale[b * p.ss_b + h * p.ss_h + blk * p.ss_blk + g] = TRITON ? sc : fmaxf(a, 0.0000001f) / 127.f;
  const bool r_unusable = TRITON && !(fabsf(r) < 3.0e38f);  // a == 0 without epsilon: the division's 0 / 0 decides

  int8_t* obase = p.out + b * p.osb + h * p.osh + blk * p.o_blk + (int64_t)tr * p.osn + tc * 8;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    uint2 w;
    if constexpr (TRITON) {
      // the exact division, for the whole 8-element chunk of the wave, only where round_half_away_pack8 asks for it
      // (~6 % of the chunks) or the reciprocal is not finite.  Bit-exact by construction.
      bool near;
      w = round_half_away_pack8(xf[i], r, near);
      if (__builtin_amdgcn_ballot_w64(near || r_unusable) != 0) {
        int q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float y = xf[i][j] / sc;  // IEEE division
          y = y + (y >= 0.f ? 0.5f : -0.5f);
          q[j] = min(max((int)y, -128), 127);  // truncation, as tl `.to(int8)`
        }
        w = make_uint2(pack_i8x4(q[0], q[1], q[2], q[3]), pack_i8x4(q[4], q[5], q[6], q[7]));
      }
    } else {
      // rint and the byte from one addition: |x r| <= 127 (1 + 3 ulp), so fl(x r) + M is M + rint(fl(x r)) exactly (ties to
      // even on both sides: M is even) and its low byte the int8 -- what (int)rintf(x * r) packs
      uint32_t tb[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) tb[j] = __float_as_uint(xf[i][j] * r + 12582912.f);
      w = make_uint2(pack_i8x4(tb[0], tb[1], tb[2], tb[3]), pack_i8x4(tb[4], tb[5], tb[6], tb[7]));
    }
    if (!RAGGED || row0 + i * RPP < p.N) *reinterpret_cast<uint2*>(obase + (int64_t)(i * RPP) * p.osn) = w;
  }
}

template <int D, bool BF16, bool TRITON, bool PER_THREAD>
__device__ __forceinline__ void k_quant_stream_walk(const QuantParams& p, const int per_wg, const int wg, const int h, const int b,
                                                    const int H, unsigned int (*gmax)[64], float (*mpart)[D]) {
  using G = QuantGeom<D, 64>;
  const int nblk = (p.N + 63) / 64, nfull = p.N / 64;  // blocks [0, nfull) are whole
  const int blk0 = wg * per_wg, blk1 = min(blk0 + per_wg, nblk);  // the host launches no empty workgroup
  if (threadIdx.x < 192) (&gmax[0][0])[threadIdx.x] = 0u;
  const uint16_t* xbase = p.x + b * p.xsb + h * p.xsh + (threadIdx.x % G::TPR) * 8;
  uint4 raw[G::NP];
  if (blk0 < nfull) k_load_rows<D, false>(xbase, p.xsn, blk0, p.N, raw);
  else k_load_rows<D, true>(xbase, p.xsn, blk0, p.N, raw);
  const uint4 mbits = quant_mean_bits<D, BF16>(p, h, b, H, wg == 0, mpart);
  int par = 0;
  for (int blk = blk0; blk < blk1; ++blk) {
    unsigned int* const zero_next = gmax[par == 0 ? 2 : par - 1];
    if (blk < nfull) {
      // the rows of the next block are requested as soon as this block's are unpacked (their registers are free then) and
      // fly during the barrier, the rounding and the stores of this block
      k_quant_block<D, BF16, TRITON, PER_THREAD, false>(p, blk, h, b, raw, mbits, gmax[par], zero_next, [&] {
        if (blk + 1 < blk1) {
          if (blk + 1 < nfull) k_load_rows<D, false>(xbase, p.xsn, blk + 1, p.N, raw);
          else k_load_rows<D, true>(xbase, p.xsn, blk + 1, p.N, raw);
        }
      });
    } else {
      k_quant_block<D, BF16, TRITON, PER_THREAD, true>(p, blk, h, b, raw, mbits, gmax[par], zero_next, [] {});  // the last
    }
    par = par == 2 ? 0 : par + 1;
  }
}

template <int D, bool BF16, bool TRITON>
__device__ __forceinline__ void k_quant_stream_body(const QuantParams& p, const int per_wg, const int wg, const int h, const int b,
                                                    const int H, unsigned int (*gmax)[64], float (*mpart)[D]) {
  // (the host admits per_block and per_thread for K: k_smooth_quant_check, kv_prepare_check)
  if (p.gran == SAGE_GRAN_PER_THREAD) k_quant_stream_walk<D, BF16, TRITON, true>(p, per_wg, wg, h, b, H, gmax, mpart);
  else k_quant_stream_walk<D, BF16, TRITON, false>(p, per_wg, wg, h, b, H, gmax, mpart);
}

// The quantizer's parameters for batch b of a call with per-batch key lengths: N and the chunk count become those of its
// len_b rows, so that the mean, the blocks and their scales are exactly those of a call on the first len_b rows (rows beyond
// are never loaded: the ragged block clamps to row len_b - 1).  The quantizers address the chunk sums of head (b, h) at
// (b H + h) S: S is count and head stride in one, but here every head has kmean_max_chunks(N) slots and the batch fills the
// first S of them -- so the base moves by `part_shift` floats, and the unchanged address arithmetic lands on the head's slots
// (the KVLEN = false instantiations keep their code).  Returns false when the workgroup, whose first 64-row block is blk0, has no
// block of the batch: it leaves before any barrier.  An empty batch has no mean to take: km = 0, not 0 / 0, stored by the
// first workgroup of the K half (k_half).
template <int D>
__device__ __forceinline__ bool kvlen_batch_params(QuantParams& p, int64_t& part_shift, const int32_t* __restrict__ kv_lens,
                                                   const int blk0, const int h, const int b, const int H, const bool k_half) {
  const int len = kv_len_of(kv_lens, b, p.N);
  if (k_half && len == 0 && blk0 == 0 && threadIdx.x < D / 8)
    *reinterpret_cast<uint4*>(p.km_out + ((int64_t)b * H + h) * D + threadIdx.x * 8) = make_uint4(0u, 0u, 0u, 0u);
  const int slots = kmean_max_chunks(p.N);
  p.N = len;
  p.S = kmean_chunks(len);
  part_shift = ((int64_t)b * H + h) * (slots - p.S) * D;
  p.mean_part += part_shift;
  return blk0 * 64 < len;
}

// KVLEN (sage_k_smooth_quant_kvlen): the grid is sized for N rows, and p becomes the batch's own (kvlen_batch_params)
template <int D, bool BF16, bool TRITON, bool KVLEN>
__global__ __launch_bounds__(256, D == 64 ? 5 : 4) void k_quant_stream_kernel(QuantParams p, const int per_wg,
                                                                              const KvLens<KVLEN> kv_lens) {
  __shared__ unsigned int gmax[3][64];
  __shared__ __attribute__((aligned(16))) float mpart[16][D];
  if constexpr (KVLEN) {
    int64_t part_shift;
    if (!kvlen_batch_params<D>(p, part_shift, kv_lens.p, blockIdx.x * per_wg, blockIdx.y, blockIdx.z, gridDim.y, true)) return;
  }
  k_quant_stream_body<D, BF16, TRITON>(p, per_wg, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.y, gmax, mpart);
}

// ------------------------------------------------------------------------------------------------
// Fused K/V pre-pass of the FP8-PV operator, at every length (a sequence is at most 16 chunks, kmean_chunk_rows): TWO launches instead of five
// (k_mean_partial, quantizer | v_stats_partial, v_stats_final, v_quant_transpose).  Every kernel below is bandwidth- or
// latency-bound and fills the chip on its own, so what the fusion saves is three launch boundaries and the ramp / tail of
// three kernels, and the VALU-heavy K quantizer shares the CUs with the bandwidth-bound V quantizer.
//   launch A  workgroups [0, S): K column sums per chunk;  [S, 2S): V per-channel max|v| per chunk
//   launch B  workgroups [0, nblk_k): K quantizer (finishes the mean itself);  the rest: V quantizer + transpose (finishes
//             max|v| itself, block 0 stores v_scale)
// Without V smoothing only max|v| is needed, which does not depend on the order of the reduction: bit-identical to
// sage_k_smooth_quant + sage_quant_v_fp8(v_mean = null).
// ------------------------------------------------------------------------------------------------
// (VPrepParams, the V half's parameter block: sage_entry.h)

template <int D, bool BF16>
__device__ __forceinline__ void v_amax_partial_body(const uint16_t* __restrict__ v, int64_t sb, int64_t sh, int64_t sn, int N,
                                                    float* __restrict__ part, int S, int s, int h, int b, int H,
                                                    float (*red)[D + 1]) {
  constexpr int TPR = D / 8, RPP = 256 / TPR;
  const int tr = threadIdx.x / TPR, tc = threadIdx.x % TPR;
  const uint16_t* base = v + b * sb + h * sh + tc * 8;
  float am[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // rows in [N, ceil16(N)) count as zeros (fused.cu:335): the same as starting at 0
  const int rows = kmean_chunk_rows(N);
  if ((s + 1) * rows <= N) {  // whole chunk: unconditional loads, eight in flight (see k_mean_partial_body)
#pragma unroll 8
    for (int i = 0; i < rows / RPP; ++i) {
      float f[8];
      unpack8<BF16>(*reinterpret_cast<const uint4*>(base + (int64_t)(s * rows + i * RPP + tr) * sn), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) am[j] = fmaxf(am[j], fabsf(f[j]));
    }
  } else {
#pragma unroll 4
    for (int i = 0; i < rows / RPP; ++i) {
      const int row = s * rows + i * RPP + tr;
      if (row < N) {
        float f[8];
        unpack8<BF16>(*reinterpret_cast<const uint4*>(base + (int64_t)row * sn), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) am[j] = fmaxf(am[j], fabsf(f[j]));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[tr][tc * 8 + j] = am[j];
  __syncthreads();
  if (threadIdx.x < D) {
    float a = red[0][threadIdx.x];
    for (int r = 1; r < RPP; ++r) a = fmaxf(a, red[r][threadIdx.x]);
    part[(((int64_t)b * H + h) * S + s) * D + threadIdx.x] = a;
  }
}

// KVLEN (see k_mean_partial_kernel): the sums and max|v| over the rows < len_b only
template <int D, bool BF16, bool KVLEN>
__global__ __launch_bounds__(256) void kv_partial_kernel(const uint16_t* __restrict__ k, int64_t ksb, int64_t ksh, int64_t ksn,
                                                         const uint16_t* __restrict__ v, int64_t vsb, int64_t vsh, int64_t vsn,
                                                         int N, float* __restrict__ kpart, float* __restrict__ vpart, int S,
                                                         const KvLens<KVLEN> kv_lens) {
  static_assert(KMEAN_ROWS == VQ_ROWS, "one chunk size for both tensors");
  __shared__ float red[256 / (D / 8)][D + 1];
  const int x = blockIdx.x;  // K chunk x, or V chunk x - S
  if constexpr (KVLEN) {
    N = kv_len_of(kv_lens.p, blockIdx.z, N);
    if ((x < S ? x : x - S) >= kmean_chunks(N)) return;
  }
  if (x < S) k_mean_partial_body<D, BF16>(k, ksb, ksh, ksn, N, kpart, S, x, blockIdx.y, blockIdx.z, gridDim.y, red);
  else v_amax_partial_body<D, BF16>(v, vsb, vsh, vsn, N, vpart, S, x - S, blockIdx.y, blockIdx.z, gridDim.y, red);
}

// The per-channel V scale of head (b, h) of H from its p.S chunk maxima (q.part): one round trip fetches all chunks (S <= 16
// <= token groups per workgroup), the FIRST token group finishes the scale and hands the coefficients over through LDS
// (every thread doing it for itself: 8 S maxima and 16 IEEE divisions per thread for 32 elements of real work), and the
// head's workgroup wg == 0 stores v_scale.  Two barriers; rcp: this thread's 8 coefficients scale_max / max|v|
template <int D>
__device__ __forceinline__ void v_scale_finish(const QuantParams& p, const VPrepParams& q, const int h, const int b, const int H,
                                               const int wg, float (*exch)[D], float (&rcp)[8]) {
  using G = VQuantGeom<D>;
  const int tg = threadIdx.x / G::TPR, tc = threadIdx.x % G::TPR;
  if (tg < p.S) {
    const float* pp = q.part + (((int64_t)b * H + h) * p.S + tg) * D + tc * 8;
    *reinterpret_cast<float4*>(&exch[tg][tc * 8]) = *reinterpret_cast<const float4*>(pp);
    *reinterpret_cast<float4*>(&exch[tg][tc * 8 + 4]) = *reinterpret_cast<const float4*>(pp + 4);
  }
  __syncthreads();
  if (tg == 0) {  // (this thread alone reads columns tc*8 .. tc*8+7 of exch, so it may overwrite them in row 0)
    float rc[8], vs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = exch[0][tc * 8 + j];
      for (int s_ = 1; s_ < p.S; ++s_) a = fmaxf(a, exch[s_][tc * 8 + j]);
      rc[j] = a > 0.f ? q.scale_max / a : 0.f;   // v_stats_final_kernel (an all-zero channel: coefficient 0, not inf)
      vs[j] = a / q.scale_max;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) exch[0][tc * 8 + j] = rc[j];
    if (wg == 0) {
      float* o = q.v_scale + ((int64_t)b * H + h) * D + tc * 8;
      *reinterpret_cast<float4*>(o) = make_float4(vs[0], vs[1], vs[2], vs[3]);
      *reinterpret_cast<float4*>(o + 4) = make_float4(vs[4], vs[5], vs[6], vs[7]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) rcp[j] = exch[0][tc * 8 + j];
}

// V half of kv_quant_kernel: unit bx (BLKS x 64 tokens) of head (b, h) of H.  p: N and the chunk count S
template <int D, bool BF16>
__device__ __forceinline__ void v_quant_unit(const QuantParams& p, const VPrepParams& q, const int bx, const int h, const int b,
                                             const int H, float (*exch)[D], uint32_t* tile) {
  // the unit's rows first: the statistics below overlap with this trip to HBM
  uint4 raw[4];
  v_quant_load<D>(q.v + b * q.sb + h * q.sh, q.sn, p.N, bx, raw);
  const float mean[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float rcp[8];
  v_scale_finish<D>(p, q, h, b, H, bx, exch, rcp);
  v_quant_to_image<D, BF16>(raw, p.N, bx, mean, rcp, tile);
  __syncthreads();
  v_quant_store_image<D>(q.out, q.ob, q.oh, q.od, q.o_tile, p.N, bx, h, b, tile);
}

// One K block or V unit per workgroup.  KVLEN (sage_kv_prepare_fp8_kvlen): the grid is sized for N rows and p, q become
// the batch's own; the V^T image of the batch's last 64-token block is written whole, its columns >= len_b as zero bytes
// (v_quant_to_image)
template <int D, bool BF16, bool TRITON, bool KVLEN>
__global__ __launch_bounds__(256, D == 64 ? 8 : 7) void kv_quant_kernel(QuantParams p, VPrepParams q, const int nblk_k,
                                                                        const KvLens<KVLEN> kv_lens) {
  using G = VQuantGeom<D>;
  __shared__ unsigned int gmax[64];
  __shared__ __attribute__((aligned(16))) float exch[16][D];  // chunk partials of this head: K sums or V max|v|
  __shared__ __attribute__((aligned(16))) uint32_t tile[G::BLKS * G::IMG];
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const bool k_half = (int)blockIdx.x < nblk_k;  // K block blockIdx.x, or V unit blockIdx.x - nblk_k (BLKS blocks)
  if constexpr (KVLEN) {
    int64_t part_shift;
    const int blk0 = k_half ? blockIdx.x : (blockIdx.x - nblk_k) * G::BLKS;
    if (!kvlen_batch_params<D>(p, part_shift, kv_lens.p, blk0, h, b, H, k_half)) return;
    q.part += part_shift;  // (the V partials have the layout of the K sums)
  }
  if (k_half) {
    quant_qk_int8_body<D, 64, BF16, TRITON>(p, blockIdx.x, h, b, H, gmax, exch);
    return;
  }
  v_quant_unit<D, BF16>(p, q, blockIdx.x - nblk_k, h, b, H, exch, tile);
}

// Launch B as a STREAMING kernel for long sequences (sage_kv_prepare_fp8 picks by the units a workgroup would walk): workgroups [0, nwg_k) walk per_k consecutive K blocks
// of their head (k_quant_stream_body), the others per_v consecutive V units (BLKS x 64 tokens), the next unit's rows
// requested while this one is transposed, the image double-buffered in LDS (one barrier per unit), and the per-channel
// scale -- S maxima and two IEEE divisions per channel -- finished ONCE per workgroup by its first token group instead of by
// every thread for every unit (three quarters of the V half's vector work otherwise).  Same arithmetic: bit-identical.
// V half of kv_quant_stream_kernel: workgroup wg of head (b, h) of H walks per_v units.  tile: two image buffers
template <int D, bool BF16>
__device__ __forceinline__ void v_quant_stream_walk(const QuantParams& p, const VPrepParams& q, const int per_v, const int wg,
                                                    const int h, const int b, const int H, float (*exch)[D],
                                                    uint32_t (*tile)[VQuantGeom<D>::BLKS * VQuantGeom<D>::IMG]) {
  using G = VQuantGeom<D>;
  const int nunits = ((p.N + 63) / 64 + G::BLKS - 1) / G::BLKS;
  const int u0 = wg * per_v, u1 = min(u0 + per_v, nunits);
  const uint16_t* vhead = q.v + b * q.sb + h * q.sh;
  uint4 raw[4];
  v_quant_load<D>(vhead, q.sn, p.N, u0, raw);
  const float mean[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float rcp[8];
  v_scale_finish<D>(p, q, h, b, H, wg, exch, rcp);
  for (int u = u0; u < u1; ++u) {
    uint32_t* img = tile[(u - u0) & 1];
    v_quant_to_image<D, BF16>(raw, p.N, u, mean, rcp, img);
    if (u + 1 < u1) v_quant_load<D>(vhead, q.sn, p.N, u + 1, raw);
    // one barrier per unit: the image buffers alternate, and the readers of this unit's buffer two units ago all passed the
    // previous unit's barrier before anyone writes it again
    __syncthreads();
    v_quant_store_image<D>(q.out, q.ob, q.oh, q.od, q.o_tile, p.N, u, h, b, img);
  }
}

// KVLEN: see kv_quant_kernel
template <int D, bool BF16, bool TRITON, bool KVLEN>
__global__ __launch_bounds__(256, D == 64 ? 5 : 4) void kv_quant_stream_kernel(QuantParams p, VPrepParams q, const int per_k,
                                                                               const int nwg_k, const int per_v,
                                                                               const KvLens<KVLEN> kv_lens) {
  using G = VQuantGeom<D>;
  __shared__ unsigned int gmax[3][64];
  __shared__ __attribute__((aligned(16))) float exch[16][D];  // chunk partials of this head: K sums or V max|v|
  __shared__ __attribute__((aligned(16))) uint32_t tile[2][G::BLKS * G::IMG];
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const bool k_half = (int)blockIdx.x < nwg_k;  // K workgroup blockIdx.x, or V workgroup blockIdx.x - nwg_k
  if constexpr (KVLEN) {
    int64_t part_shift;
    const int blk0 = k_half ? (int)blockIdx.x * per_k : (int)(blockIdx.x - nwg_k) * per_v * G::BLKS;
    if (!kvlen_batch_params<D>(p, part_shift, kv_lens.p, blk0, h, b, H, k_half)) return;
    q.part += part_shift;  // (the V partials have the layout of the K sums)
  }
  if (k_half) {
    k_quant_stream_body<D, BF16, TRITON>(p, per_k, blockIdx.x, h, b, H, gmax, exch);
    return;
  }
  v_quant_stream_walk<D, BF16>(p, q, per_v, blockIdx.x - nwg_k, h, b, H, exch, tile);
}

// ------------------------------------------------------------------------------------------------
// Persistent KV cache (include/sageattn_hip_kvcache.h): extend prepared operands in place, one launch.
//   workgroups [0, k_slots): K slot i is tile t0_b + i of the batch, quantized by k_quant_block against the FROZEN km (read
//                            straight from p.k.mean: no chunk sums), ragged at len_b where the tile holds row len_b - 1
//   the rest (WITH_V):       V slot i is unit t0_b / BLKS + i (BLKS 64-token blocks), v_quant_transpose_body with the frozen
//                            coefficients, clamped to +-448 (later rows may exceed a frozen range)
// t0_b = floor(min(start_b, len_b - 1) / 64).  A slot beyond the batch's last tile, and every slot of an empty batch, leaves
// before any barrier.  Same arithmetic per tile as the quantizers above: bit-identical to a from-scratch quantization of the
// first len_b rows against km / v_coef.
// ------------------------------------------------------------------------------------------------
struct KvAppendParams {
  QuantParams k;        // x = k, mean = km, out = k8, scale; N = the capacity
  VPrepParams v;        // v, out = the V^T image (o_tile 64); part, v_scale, scale_max unused
  const float* v_coef;  // [B,H,2,D]: zeros, coefficients
  const int32_t* start_lens;
  const int32_t* kv_lens;
  int k_slots;
};

template <int D, bool BF16, bool TRITON, bool PER_THREAD>
__device__ __forceinline__ void kv_append_k_tile(const QuantParams& p, const int blk, const int h, const int b, const int H,
                                                 unsigned int (*gmax)[64]) {
  using G = QuantGeom<D, 64>;
  if (threadIdx.x < 64) gmax[0][threadIdx.x] = 0u;
  const int tc = (int)threadIdx.x % G::TPR;
  const uint16_t* xbase = p.x + b * p.xsb + h * p.xsh + tc * 8;
  const bool whole = blk < p.N / 64;
  uint4 raw[G::NP];
  if (whole) k_load_rows<D, false>(xbase, p.xsn, blk, p.N, raw);
  else k_load_rows<D, true>(xbase, p.xsn, blk, p.N, raw);
  const uint4 mbits = *reinterpret_cast<const uint4*>(p.mean + ((int64_t)b * H + h) * D + tc * 8);
  __syncthreads();  // gmax zeroed
  // (zero_next: the streaming walk's rotation has nothing to prepare here; a second buffer takes the store)
  if (whole) k_quant_block<D, BF16, TRITON, PER_THREAD, false>(p, blk, h, b, raw, mbits, gmax[0], gmax[1], [] {});
  else k_quant_block<D, BF16, TRITON, PER_THREAD, true>(p, blk, h, b, raw, mbits, gmax[0], gmax[1], [] {});
}

// The block table of the paged form (include/sageattn_hip_paged.h): row b, `stride` int32 entries, names the pages of batch b;
// a page holds 1 << shift tiles.  The K, V, INT8 K, scale and V^T pointers of KvAppendParams are then POOLS whose batch strides
// (xsb, osb, ss_b; sb, ob) are the strides of a page, and k.N the logical capacity max_pages * page_size.
struct KvPageTable {
  const int32_t* table;
  int64_t stride;
  int shift;
};
// the page of logical tile `blk` of batch b: only tiles below ceil(len_b / 64) are asked for, so no entry at or beyond
// ceil(len_b / page_size) is read
__device__ __forceinline__ int64_t kv_page_of(const KvPageTable& pt, const int b, const int blk) {
  return pt.table[(int64_t)b * pt.stride + (blk >> pt.shift)];
}

// V unit of the paged form: v_quant_transpose_body with the rows and the image blocks looked up per 64-token block.  At
// head_dim 64 a unit is two blocks, which with 64-key pages lie in two pages: the two halves of the workgroup look up their
// own.  A row index clamped to len - 1 (the loads are unconditional, as in v_quant_load) lies in block min(blk, ntile - 1): a
// block the batch has, whose page is named.
template <int D, bool BF16>
__device__ __forceinline__ void kv_append_v_unit_paged(const VPrepParams& q, const KvPageTable& pt, const int len,
                                                       const float (&mean)[8], const float (&rcp)[8], const int unit,
                                                       const int h, const int b, uint32_t* __restrict__ tile) {
  using G = VQuantGeom<D>;
  const int tmask = (1 << pt.shift) - 1, ntile = (len + 63) >> 6;
  uint4 raw[4];
  {
    const int tg = threadIdx.x / G::TPR, tc = threadIdx.x % G::TPR;
    const int blk = unit * G::BLKS + tg / 16, blk_c = min(blk, ntile - 1);
    const uint16_t* vbase = q.v + kv_page_of(pt, b, blk_c) * q.sb + h * q.sh + (int64_t)((blk_c & tmask) * 64) * q.sn + tc * 8;
    const int row0 = blk * 64 + 4 * (tg % 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) raw[i] = *reinterpret_cast<const uint4*>(vbase + (int64_t)(min(row0 + i, len - 1) & 63) * q.sn);
  }
  v_quant_to_image<D, BF16, true>(raw, len, unit, mean, rcp, tile);
  __syncthreads();
  for (int c = threadIdx.x; c < G::BLKS * D * 4; c += 256) {
    const int bo = c / (D * 4), cc = c % (D * 4), d = cc >> 2, ch = cc & 3;
    const int ob_blk = unit * G::BLKS + bo;
    if (ob_blk * 64 >= len) continue;
    const uint4 u = *reinterpret_cast<const uint4*>(&tile[bo * G::IMG + d * 16 + 4 * (d >> 3) + ch * 4]);
    *reinterpret_cast<uint4*>(q.out + kv_page_of(pt, b, ob_blk) * q.ob + h * q.oh + (int64_t)d * q.od + (ob_blk & tmask) * q.o_tile +
                              ch * 16) = u;
  }
}

template <int D, bool BF16, bool TRITON, bool WITH_V>
__global__ __launch_bounds__(256, D == 64 ? 5 : 4) void kv_cache_append_kernel(const KvAppendParams a) {
  using G = VQuantGeom<D>;
  __shared__ unsigned int gmax[2][64];
  __shared__ __attribute__((aligned(16))) uint32_t tile[WITH_V ? G::BLKS * G::IMG : 4];
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const int len = kv_len_of(a.kv_lens, b, a.k.N);
  if (len == 0) return;
  const int t0 = min(kv_len_of(a.start_lens, b, a.k.N), len - 1) >> 6;
  const int ntile = (len + 63) >> 6;
  if ((int)blockIdx.x < a.k_slots) {
    const int blk = t0 + blockIdx.x;
    if (blk >= ntile) return;
    QuantParams p = a.k;
    p.N = len;
    if (p.gran == SAGE_GRAN_PER_THREAD) kv_append_k_tile<D, BF16, TRITON, true>(p, blk, h, b, H, gmax);
    else kv_append_k_tile<D, BF16, TRITON, false>(p, blk, h, b, H, gmax);
    return;
  }
  if constexpr (WITH_V) {
    const int unit = t0 / G::BLKS + ((int)blockIdx.x - a.k_slots);
    if (unit * G::BLKS >= ntile) return;
    const int tc = threadIdx.x % G::TPR;
    float mean[8], rcp[8];
    {
      const float* cf = a.v_coef + (((int64_t)b * H + h) * 2) * D + tc * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) { mean[j] = cf[j]; rcp[j] = cf[D + j]; }
    }
    v_quant_transpose_body<D, BF16, true>(a.v.v, a.v.sb, a.v.sh, a.v.sn, len, mean, rcp, a.v.out, a.v.ob, a.v.oh, a.v.od, a.v.o_tile,
                                    unit, h, b, tile);
  }
}

// The paged form (sage_kv_cache_append_paged): the same grid, the same slots in logical tiles, the same K block and V unit
// bodies.  A K slot moves its pointers to the page of its tile -- after that, tile `blk` of batch b IS the tile of the page,
// and kv_append_k_tile runs unchanged (km stays that of batch b); a V slot runs kv_append_v_unit_paged.
// (A kernel text of its own: with the slot arithmetic shared through one function template and a PAGED flag, the 16
//  instantiations of kv_cache_append_kernel came out with other instruction streams, 2 to 105 instructions shorter.)
template <int D, bool BF16, bool TRITON, bool WITH_V>
__global__ __launch_bounds__(256, D == 64 ? 5 : 4) void kv_cache_append_paged_kernel(const KvAppendParams a, const KvPageTable pt) {
  using G = VQuantGeom<D>;
  __shared__ unsigned int gmax[2][64];
  __shared__ __attribute__((aligned(16))) uint32_t tile[WITH_V ? G::BLKS * G::IMG : 4];
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const int len = kv_len_of(a.kv_lens, b, a.k.N);
  if (len == 0) return;
  const int t0 = min(kv_len_of(a.start_lens, b, a.k.N), len - 1) >> 6;
  const int ntile = (len + 63) >> 6;
  if ((int)blockIdx.x < a.k_slots) {
    const int blk = t0 + blockIdx.x;
    if (blk >= ntile) return;
    QuantParams p = a.k;
    p.N = len;
    const int64_t page = kv_page_of(pt, b, blk);
    const int64_t back = (blk & ((1 << pt.shift) - 1)) - blk;  // tile inside the page - logical tile (<= 0)
    p.x += page * p.xsb + back * 64 * p.xsn - b * p.xsb;
    p.out += page * p.osb + back * p.o_blk - b * p.osb;
    p.scale += page * p.ss_b + back * p.ss_blk - b * p.ss_b;
    if (p.gran == SAGE_GRAN_PER_THREAD) kv_append_k_tile<D, BF16, TRITON, true>(p, blk, h, b, H, gmax);
    else kv_append_k_tile<D, BF16, TRITON, false>(p, blk, h, b, H, gmax);
    return;
  }
  if constexpr (WITH_V) {
    const int unit = t0 / G::BLKS + ((int)blockIdx.x - a.k_slots);
    if (unit * G::BLKS >= ntile) return;
    const int tc = threadIdx.x % G::TPR;
    float mean[8], rcp[8];
    {
      const float* cf = a.v_coef + (((int64_t)b * H + h) * 2) * D + tc * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) { mean[j] = cf[j]; rcp[j] = cf[D + j]; }
    }
    kv_append_v_unit_paged<D, BF16>(a.v, pt, len, mean, rcp, unit, h, b, tile);
  }
}

// ------------------------------------------------------------------------------------------------
// The paged cache without fp16 pools (include/sageattn_hip_paged_rows.h, sage_kv_cache_append_rows_paged): the same grid and
// the same slots in logical tiles as kv_cache_append_paged_kernel, but the rows come from the step's k_new / v_new [B,H,T,D]
// (logical row s_b + i is row i) and, for the rows of tile t0_b below min(s_b, len_b), from the ring k_tail [B,H,2,64,D] (row
// r in slot (r >> 6) & 1, row r & 63).  Rows of k_new / v_new at i >= n_b = min(len_b - s_b, T) are never loaded: every row
// index is clamped into [0, n_b), and a unit without new rows loads none.
//
// THE RING HAS ONE READER AND ONE WRITER: K slot 0 of (b, h).  Only tile t0_b has rows below s_b (a later tile starts at
// 64 * (t0_b + 1) > s_b, and with s_b >= len_b there is no later tile), so only slot 0 reads the ring; the same workgroup
// writes the new rows of the tiles tl_b and tl_b - 1 into it AFTER it has quantized its tile.  With a chunk of more than 64
// rows tl_b can have the parity of t0_b, and the rows written are then the rows read -- which is why no other workgroup
// writes them: nothing orders workgroups.  Inside the workgroup the order holds because every thread's ring rows feed the
// group maxima it publishes (atomicMax into LDS) in front of the barrier of k_quant_block -- a load has returned before its
// value is used -- so behind that barrier (and the one in front of the ring's stores) every ring row of the workgroup sits
// in registers.
// V_MODE 1 (FP8 P.V): the V unit quantizes the new rows into the LDS image with v_quant_to_image<.., SAT = true>, zeros for
// the columns >= len_b, and stores it 16 bytes at a time; a chunk with tokens below min(s_b, len_b) -- four consecutive tokens
// share a dword, in the image's permuted order -- takes those BYTES from the chunk the pool holds, and a chunk of old tokens
// alone is not stored.  V_MODE 0 (FP16 / BF16 P.V): the rows [s_b, len_b) of v_new are copied into the pages of v_pool.
// ------------------------------------------------------------------------------------------------
struct KvRowsParams {
  const uint16_t* k_new;  // [B,H,T,D], strides in elements
  int64_t ksb, ksh, ksn;
  const uint16_t* v_new;
  int64_t vsb, vsh, vsn;
  uint16_t* k_tail;       // [B,H,2,64,D] contiguous
  uint16_t* v_pool;       // V_MODE 0: [P,H,page_size,D]
  int64_t vpb, vph, vpn;
  int T;
};

// the 64 rows of tile `blk`: rows below `keep` out of the ring slot of the tile, the others out of k_new (row - s); rows past
// the end read row len - 1, as k_load_rows<CLAMP> (the caller ignores them).  A row at or above keep has 0 <= row - s < n.
template <int D>
__device__ __forceinline__ void k_load_rows_ring(const uint16_t* knew, const int64_t ksn, const uint16_t* ring_slot, const int blk,
                                                 const int keep, const int s, const int n, const int len,
                                                 uint4 (&raw)[QuantGeom<D, 64>::NP]) {
  using G = QuantGeom<D, 64>;
  const int row0 = blk * 64 + (int)threadIdx.x / G::TPR;
#pragma unroll
  for (int i = 0; i < G::NP; ++i) {
    const int row = min(row0 + i * G::RPP, len - 1);
    const uint16_t* src = row < keep ? ring_slot + (row & 63) * D : knew + (int64_t)max(min(row - s, n - 1), 0) * ksn;
    raw[i] = *reinterpret_cast<const uint4*>(src);
  }
}

template <int D, bool BF16, bool TRITON, bool PER_THREAD>
__device__ __forceinline__ void kv_rows_k_tile(const QuantParams& p, const uint16_t* knew, const int64_t ksn,
                                               const uint16_t* ring_slot, const int blk, const int keep, const int s, const int n,
                                               const int h, const int b, const int H, unsigned int (*gmax)[64]) {
  using G = QuantGeom<D, 64>;
  if (threadIdx.x < 64) gmax[0][threadIdx.x] = 0u;
  const int tc = (int)threadIdx.x % G::TPR;
  uint4 raw[G::NP];
  k_load_rows_ring<D>(knew + tc * 8, ksn, ring_slot + tc * 8, blk, keep, s, n, p.N, raw);
  const uint4 mbits = *reinterpret_cast<const uint4*>(p.mean + ((int64_t)b * H + h) * D + tc * 8);
  __syncthreads();  // gmax zeroed
  if (blk < p.N / 64) k_quant_block<D, BF16, TRITON, PER_THREAD, false>(p, blk, h, b, raw, mbits, gmax[0], gmax[1], [] {});
  else k_quant_block<D, BF16, TRITON, PER_THREAD, true>(p, blk, h, b, raw, mbits, gmax[0], gmax[1], [] {});
}

template <int D, bool BF16, bool TRITON, int V_MODE>
__global__ __launch_bounds__(256, D == 64 ? 5 : 4) void kv_cache_append_rows_paged_kernel(const KvAppendParams a, const KvPageTable pt,
                                                                                          const KvRowsParams r) {
  using G = VQuantGeom<D>;
  __shared__ unsigned int gmax[2][64];
  __shared__ __attribute__((aligned(16))) uint32_t tile[V_MODE == 1 ? G::BLKS * G::IMG : 4];
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const int len = kv_len_of(a.kv_lens, b, a.k.N);
  if (len == 0) return;
  const int s = kv_len_of(a.start_lens, b, a.k.N);
  const int keep = min(s, len);                // rows below are the cache's own
  const int n = min(max(len - s, 0), r.T);     // rows of k_new / v_new that may be loaded
  const int t0 = min(s, len - 1) >> 6;
  const int ntile = (len + 63) >> 6;
  const int tmask = (1 << pt.shift) - 1;
  if ((int)blockIdx.x < a.k_slots) {
    const int blk = t0 + blockIdx.x;
    if (blk >= ntile) return;
    QuantParams p = a.k;
    p.N = len;
    const int64_t page = kv_page_of(pt, b, blk);
    const int64_t back = (blk & tmask) - blk;  // tile inside the page - logical tile (<= 0)
    p.out += page * p.osb + back * p.o_blk - b * p.osb;
    p.scale += page * p.ss_b + back * p.ss_blk - b * p.ss_b;
    const uint16_t* knew = r.k_new + b * r.ksb + h * r.ksh;
    uint16_t* ring = r.k_tail + ((int64_t)b * H + h) * (2 * 64 * D);
    const int keep_here = blockIdx.x == 0 ? keep : 0;  // slot 0 alone reads the ring
    if (p.gran == SAGE_GRAN_PER_THREAD)
      kv_rows_k_tile<D, BF16, TRITON, true>(p, knew, r.ksn, ring + (blk & 1) * 64 * D, blk, keep_here, s, n, h, b, H, gmax);
    else
      kv_rows_k_tile<D, BF16, TRITON, false>(p, knew, r.ksn, ring + (blk & 1) * 64 * D, blk, keep_here, s, n, h, b, H, gmax);
    if (blockIdx.x != 0) return;
    // ... and alone writes it: the rows of [s, len) that lie in the tiles tl - 1 and tl (at most 128)
    __syncthreads();
    const int lo = max(s, 64 * (ntile - 2));
    const int cnt = (len - lo) * (D / 8);  // <= 0: no new rows
    for (int c = threadIdx.x; c < cnt; c += 256) {
      const int row = lo + c / (D / 8), col = (c % (D / 8)) * 8;
      const uint4 u = *reinterpret_cast<const uint4*>(knew + (int64_t)min(row - s, n - 1) * r.ksn + col);
      *reinterpret_cast<uint4*>(ring + (row & 127) * D + col) = u;
    }
    return;
  }
  const int unit = t0 / G::BLKS + ((int)blockIdx.x - a.k_slots);
  if (unit * G::BLKS >= ntile || (n == 0 && V_MODE == 0)) return;
  const int tg = threadIdx.x / G::TPR, tc = threadIdx.x % G::TPR;
  const int blk = unit * G::BLKS + tg / 16, row0 = blk * 64 + 4 * (tg % 16);
  const uint16_t* vnew = r.v_new + b * r.vsb + h * r.vsh + tc * 8;
  if constexpr (V_MODE == 0) {
    if (row0 >= len || row0 + 4 <= s) return;
    uint16_t* dst = r.v_pool + kv_page_of(pt, b, blk) * r.vpb + h * r.vph + (int64_t)((blk & tmask) * 64) * r.vpn + tc * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + i;
      if (row >= s && row < len && row - s < n)
        *reinterpret_cast<uint4*>(dst + (int64_t)(row & 63) * r.vpn) = *reinterpret_cast<const uint4*>(vnew + (int64_t)(row - s) * r.vsn);
    }
  } else {
    float mean[8], rcp[8];
    {
      const float* cf = a.v_coef + (((int64_t)b * H + h) * 2) * D + tc * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) { mean[j] = cf[j]; rcp[j] = cf[D + j]; }
    }
    uint4 raw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      raw[i] = make_uint4(0u, 0u, 0u, 0u);  // (rows below keep are replaced by the pool's bytes, rows >= len become zeros)
      if (n > 0) raw[i] = *reinterpret_cast<const uint4*>(vnew + (int64_t)max(min(row0 + i - s, n - 1), 0) * r.vsn);
    }
    v_quant_to_image<D, BF16, true>(raw, len, unit, mean, rcp, tile);
    __syncthreads();
    for (int c = threadIdx.x; c < G::BLKS * D * 4; c += 256) {
      const int bo = c / (D * 4), cc = c % (D * 4), d = cc >> 2, ch = cc & 3;
      const int ob_blk = unit * G::BLKS + bo;
      if (ob_blk * 64 >= len) continue;
      // dword k of chunk ch holds the tokens tok0 + 8 k .. + 3 of the block, byte i token + i (v_quant_to_image)
      const int old0 = keep - (ob_blk * 64 + 32 * (ch & 1) + 4 * (ch >> 1));  // old tokens of dword k: clamp(old0 - 8 k, 0, 4)
      if (old0 >= 28) continue;                                                // a chunk of old tokens alone
      uint4 u = *reinterpret_cast<const uint4*>(&tile[bo * G::IMG + d * 16 + 4 * (d >> 3) + ch * 4]);
      uint8_t* dst = a.v.out + kv_page_of(pt, b, ob_blk) * a.v.ob + h * a.v.oh + (int64_t)d * a.v.od + (ob_blk & tmask) * a.v.o_tile + ch * 16;
      if (old0 > 0) {
        const uint4 o = *reinterpret_cast<const uint4*>(dst);
        const auto mix = [&](uint32_t nw, uint32_t ol, int k) {
          const int no = min(max(old0 - 8 * k, 0), 4);
          const uint32_t m = no >= 4 ? 0xffffffffu : (1u << (8 * no)) - 1u;
          return (ol & m) | (nw & ~m);
        };
        u = make_uint4(mix(u.x, o.x, 0), mix(u.y, o.y, 1), mix(u.z, o.z, 2), mix(u.w, o.w, 3));
      }
      *reinterpret_cast<uint4*>(dst) = u;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// K2: sub_mean_f16
// ------------------------------------------------------------------------------------------------
template <bool BF16>
__global__ __launch_bounds__(256) void sub_mean_f16_kernel(const uint16_t* __restrict__ v, int64_t sb, int64_t sh,
                                                           int64_t sn, const uint16_t* __restrict__ vm,
                                                           uint16_t* __restrict__ out, int64_t ob, int64_t oh,
                                                           int64_t on, int N, int D) {
  const int TPR = D / 8, RPP = 256 / TPR;
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const int tr = threadIdx.x / TPR, tc = threadIdx.x % TPR;
  const int row = blockIdx.x * RPP + tr;
  if (row >= N) return;
  float m[8], x[8];
  unpack8<BF16>(*reinterpret_cast<const uint4*>(vm + ((int64_t)b * H + h) * D + tc * 8), m);
  unpack8<BF16>(*reinterpret_cast<const uint4*>(v + b * sb + h * sh + (int64_t)row * sn + tc * 8), x);
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // packed subtraction in the input dtype (fused.cu:233), then fp16 (:235-238)
    const float lo = round_to_elem<BF16>(x[2 * j] - m[2 * j]);
    const float hi = round_to_elem<BF16>(x[2 * j + 1] - m[2 * j + 1]);
    w[j] = (uint32_t)f32_to_elem_bits<false>(lo) | ((uint32_t)f32_to_elem_bits<false>(hi) << 16);
  }
  *reinterpret_cast<uint4*>(out + b * ob + h * oh + (int64_t)row * on + tc * 8) = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- host side (sage_entry.h): checks that fill the parameters, then the launches -----------------------------------------

// Units (64-row K blocks, V units) per workgroup of a streaming quantizer: as many as leave about `target` workgroups for
// all B*H heads, at most `cap`, and at least one.
static int units_per_wg(int64_t BH, int units, int64_t target, int64_t cap) {
  int64_t per = (BH * units + target - 1) / target;
  per = per > cap ? cap : per;
  return (int)(per < 1 ? 1 : per > units ? units : per);
}

// `slots` chunk slots per head: the chunks of N rows or, with kv_lens, kmean_max_chunks(N) (every batch is chunked by its
// own length)
static void launch_k_mean_partial(const sage_tensor& k, int B, int H, int N, int D, bool bf16, float* part, int slots,
                                  const int32_t* kv_lens, hipStream_t st) {
  by_dim(D, [&](auto d) {
    by_flag(bf16, [&](auto bf) {
      by_flag(kv_lens != nullptr, [&](auto kl) {
        hipLaunchKernelGGL((k_mean_partial_kernel<decltype(d)::value, decltype(bf)::value, decltype(kl)::value>),
                           dim3(slots, H, B), dim3(256), 0, st, (const uint16_t*)k.data, k.stride_b, k.stride_h, k.stride_n, N,
                           part, slots, kv_lens);
      });
    });
  });
}

int quant_check(QuantCall& c, const sage_tensor* x, int dtype, int B, int H, int N, int D, const void* mean,
                const sage_tensor* out, float* scale, int gran, int is_key, int blk, int warp, float mult, int rounding,
                const void* lse_dot_vec, int dot_group, float* lse_dot, const QuantOptions& opt) {
  if (!tensor_ok(x, 8) || !tensor_ok(out, 8) || !scale || B <= 0 || H <= 0 || N <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = dim_dtype_status(D, dtype)) return s;
  if (gran < SAGE_GRAN_PER_BLOCK || gran > SAGE_GRAN_PER_THREAD) return SAGE_ERR_INVALID_ARGUMENT;
  if (rounding != SAGE_ROUND_TRITON && rounding != SAGE_ROUND_CUDA) return SAGE_ERR_INVALID_ARGUMENT;
  if (blk != 64 && blk != 128) return SAGE_ERR_INVALID_ARGUMENT;
  if (gran == SAGE_GRAN_PER_BLOCK) warp = blk;
  if ((warp != 16 && warp != 32 && warp != 64 && warp != 128) || blk % warp != 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (mean && !aligned16(mean)) return SAGE_ERR_INVALID_ARGUMENT;
  if (opt.mean_part && (opt.S < 1 || opt.S > 16 || !aligned16(opt.mean_part))) return SAGE_ERR_INVALID_ARGUMENT;  // mpart[16][D] in the kernel
  if ((lse_dot_vec != nullptr) != (lse_dot != nullptr)) return SAGE_ERR_INVALID_ARGUMENT;
  if (lse_dot_vec && (dot_group <= 0 || H % dot_group != 0 || !aligned16(lse_dot_vec))) return SAGE_ERR_INVALID_ARGUMENT;
  const int nblk = (N + blk - 1) / blk;
  const int gpb = gran == SAGE_GRAN_PER_BLOCK ? 1 : gran == SAGE_GRAN_PER_WARP ? blk / warp : (blk / warp) * (is_key ? 4 : 8);
  if (gpb > 64) return SAGE_ERR_INVALID_ARGUMENT;
  QuantParams& p = c.p;
  p.x = (const uint16_t*)x->data; p.xsb = x->stride_b; p.xsh = x->stride_h; p.xsn = x->stride_n;
  p.mean = (const uint16_t*)mean;
  p.out = (int8_t*)out->data; p.osb = out->stride_b; p.osh = out->stride_h; p.osn = out->stride_n;
  p.scale = scale; p.dot_vec = (const uint16_t*)lse_dot_vec; p.dot_out = lse_dot; p.dot_group = dot_group > 0 ? dot_group : 1;
  p.cu = opt.cu;
  p.mean_part = opt.mean_part; p.S = opt.S; p.km_out = (uint16_t*)opt.km_out;
  p.o_blk = opt.out_blk_stride ? opt.out_blk_stride : (int64_t)blk * out->stride_n;
  p.ss_b = opt.scale_strides ? opt.scale_strides[0] : (int64_t)H * nblk * gpb;
  p.ss_h = opt.scale_strides ? opt.scale_strides[1] : (int64_t)nblk * gpb;
  p.ss_blk = opt.scale_strides ? opt.scale_strides[2] : gpb;
  if (opt.out_blk_stride < 0 || (opt.out_blk_stride & 7) || p.ss_blk < gpb) return SAGE_ERR_INVALID_ARGUMENT;
  p.N = N; p.G = nblk * gpb; p.gran = gran; p.is_key = is_key ? 1 : 0; p.warp = warp; p.mult = mult; p.rounding = rounding;
  p.warp_shift = warp == 16 ? 4 : warp == 32 ? 5 : warp == 64 ? 6 : 7;
  c.B = B; c.H = H; c.D = D; c.blk = blk; c.bf16 = dtype == SAGE_BF16;
  return SAGE_OK;
}

int quant_launch(const QuantCall& c, hipStream_t st) {
  const dim3 grid((c.p.N + c.blk - 1) / c.blk, c.H, c.B);
  launch_begin();
  by_dim(c.D, [&](auto d) {
    by_flag(c.blk == 128, [&](auto b128) {
      by_flag(c.bf16, [&](auto bf) {
        by_flag(c.p.rounding == SAGE_ROUND_TRITON, [&](auto tr) {
          constexpr int BLK = decltype(b128)::value ? 128 : 64;
          hipLaunchKernelGGL((quant_qk_int8_kernel<decltype(d)::value, BLK, decltype(bf)::value, decltype(tr)::value>), grid,
                             dim3(256), 0, st, c.p);
        });
      });
    });
  });
  return launch_status();
}

int k_smooth_quant_check(KSmoothCall& c, const sage_tensor* k, int dtype, int B, int H, int N, int D, const sage_tensor* out,
                         float* scale, void* km, int gran, int rounding, void* workspace, const int32_t* kv_lens) {
  if (!km || !workspace || (kv_lens && !aligned16(km))) return SAGE_ERR_INVALID_ARGUMENT;  // (km = 0 of an empty batch: 16-byte stores)
  if (gran != SAGE_GRAN_PER_BLOCK && gran != SAGE_GRAN_PER_THREAD) return SAGE_ERR_INVALID_ARGUMENT;
  if (!tensor_ok(k, 8) || B <= 0 || H <= 0 || N <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = dim_dtype_status(D, dtype)) return s;
  QuantOptions opt;
  opt.mean_part = c.part = (float*)workspace;
  opt.S = kmean_chunks(N);
  opt.km_out = km;
  if (const int s = quant_check(c.q, k, dtype, B, H, N, D, nullptr, out, scale, gran, 1, 64, 64, 1.0f, rounding, nullptr, 1,
                                nullptr, opt))
    return s;
  c.k = *k;
  c.kv_lens = kv_lens;
  c.slots = kv_lens ? kmean_max_chunks(N) : opt.S;
  // as many blocks per workgroup as leave about as many workgroups per CU as the quantizer's registers allow to be resident
  // (five at head_dim 64, four at 128), so that every workgroup is resident from the start and streams its share of a head
  const int nblk = (N + 63) / 64;
  c.per_wg = units_per_wg((int64_t)B * H, nblk, 256 * (D == 64 ? 5 : 4), nblk);
  return SAGE_OK;
}

int k_smooth_quant_launch(const KSmoothCall& c, hipStream_t st) {
  const QuantParams& p = c.q.p;
  launch_begin();
  launch_k_mean_partial(c.k, c.q.B, c.q.H, p.N, c.q.D, c.q.bf16, c.part, c.slots, c.kv_lens, st);
  if (launch_status() != SAGE_OK) return SAGE_ERR_LAUNCH;
  const int nblk = (p.N + 63) / 64;
  const dim3 grid((nblk + c.per_wg - 1) / c.per_wg, c.q.H, c.q.B);
  launch_begin();
  by_dim(c.q.D, [&](auto d) {
    by_flag(c.q.bf16, [&](auto bf) {
      by_flag(p.rounding == SAGE_ROUND_TRITON, [&](auto tr) {
        by_flag(c.kv_lens != nullptr, [&](auto kl) {
          hipLaunchKernelGGL((k_quant_stream_kernel<decltype(d)::value, decltype(bf)::value, decltype(tr)::value, decltype(kl)::value>),
                             grid, dim3(256), 0, st, p, c.per_wg, c.kv_lens);
        });
      });
    });
  });
  return launch_status();
}

int kv_prepare_check(KVPrepCall& c, const sage_tensor* k, const sage_tensor* v, int dtype, int B, int H, int N, int D,
                     const sage_tensor* k_int8, float* k_scale, void* km, int gran, int rounding, const sage_tensor* v_fp8,
                     float* v_scale, float scale_max, void* workspace, const int32_t* kv_lens) {
  if (!km || !workspace || !v_scale || !(scale_max > 0.f)) return SAGE_ERR_INVALID_ARGUMENT;
  if (kv_lens && !aligned16(km)) return SAGE_ERR_INVALID_ARGUMENT;  // (km = 0 of an empty batch: 16-byte stores)
  if (gran != SAGE_GRAN_PER_BLOCK && gran != SAGE_GRAN_PER_THREAD) return SAGE_ERR_INVALID_ARGUMENT;
  if (!tensor_ok(k, 8) || !tensor_ok(v, 8) || B <= 0 || H <= 0 || N <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (!tensor_ok(v_fp8, 16)) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = dim_dtype_status(D, dtype)) return s;
  const int S = kmean_chunks(N);
  c.slots = kv_lens ? kmean_max_chunks(N) : S;  // chunk slots per head (every batch is chunked by its own length)
  c.kpart = (float*)workspace;
  c.vpart = c.kpart + (size_t)B * H * c.slots * D;
  c.kv_lens = kv_lens;
  QuantOptions opt;
  opt.mean_part = c.kpart;
  opt.S = S;
  opt.km_out = km;
  if (const int s = quant_check(c.k, k, dtype, B, H, N, D, nullptr, k_int8, k_scale, gran, 1, 64, 64, 1.0f, rounding, nullptr,
                                1, nullptr, opt))
    return s;
  VPrepParams& q = c.v;
  q.v = (const uint16_t*)v->data; q.sb = v->stride_b; q.sh = v->stride_h; q.sn = v->stride_n;
  q.out = (uint8_t*)v_fp8->data; q.ob = v_fp8->stride_b; q.oh = v_fp8->stride_h; q.od = v_fp8->stride_n; q.o_tile = 64;
  q.v_scale = v_scale; q.part = c.vpart; q.scale_max = scale_max;
  c.nblk_k = (N + 63) / 64;
  const int blks = by_dim(D, [](auto d) { return VQuantGeom<decltype(d)::value>::BLKS; });
  c.nunit_v = (c.nblk_k + blks - 1) / blks;
  // each half gets about half of the workgroups the chip holds at once (as sage_k_smooth_quant), with at most 32 units per
  // workgroup: beyond, more generations of workgroups measured better than longer walks
  const int64_t target = 128 * (D == 64 ? 5 : 4), cap = 32;
  c.per_k = units_per_wg((int64_t)B * H, c.nblk_k, target, cap);
  c.per_v = units_per_wg((int64_t)B * H, c.nunit_v, target, cap);
  // Streaming pays where a workgroup walks enough units to hide its start-up (measured, tools/prepass_ab.py, B*H = 128: head_dim
  // 128: 4-8 units per workgroup +6..10 % slower than one unit per workgroup, 16-32 units 6-12 % faster, 64 even; head_dim 64:
  // 2 units slower, 4 faster); below that the one-unit-per-workgroup kernel (seven or eight workgroups per CU) runs.
  c.streaming = c.per_v >= (D == 64 ? 4 : 12);
  return SAGE_OK;
}

int kv_prepare_launch(const KVPrepCall& c, hipStream_t st) {
  const QuantParams& p = c.k.p;
  const VPrepParams& q = c.v;
  const int B = c.k.B, H = c.k.H;
  launch_begin();
  by_dim(c.k.D, [&](auto d) {
    by_flag(c.k.bf16, [&](auto bf) {
      by_flag(c.kv_lens != nullptr, [&](auto kl) {
        hipLaunchKernelGGL((kv_partial_kernel<decltype(d)::value, decltype(bf)::value, decltype(kl)::value>),
                           dim3(2 * c.slots, H, B), dim3(256), 0, st, p.x, p.xsb, p.xsh, p.xsn, q.v, q.sb, q.sh, q.sn, p.N, c.kpart,
                           c.vpart, c.slots, c.kv_lens);
      });
    });
  });
  if (launch_status() != SAGE_OK) return SAGE_ERR_LAUNCH;
  const int nwg_k = (c.nblk_k + c.per_k - 1) / c.per_k, nwg_v = (c.nunit_v + c.per_v - 1) / c.per_v;
  by_dim(c.k.D, [&](auto d) {
    by_flag(c.k.bf16, [&](auto bf) {
      by_flag(p.rounding == SAGE_ROUND_TRITON, [&](auto tr) {
        by_flag(c.kv_lens != nullptr, [&](auto kl) {
          constexpr int DD = decltype(d)::value;
          constexpr bool BF = decltype(bf)::value, TR = decltype(tr)::value, KL = decltype(kl)::value;
          if (c.streaming)
            hipLaunchKernelGGL((kv_quant_stream_kernel<DD, BF, TR, KL>), dim3(nwg_k + nwg_v, H, B), dim3(256), 0, st, p, q, c.per_k,
                               nwg_k, c.per_v, c.kv_lens);
          else
            hipLaunchKernelGGL((kv_quant_kernel<DD, BF, TR, KL>), dim3(c.nblk_k + c.nunit_v, H, B), dim3(256), 0, st, p, q,
                               c.nblk_k, c.kv_lens);
        });
      });
    });
  });
  return launch_status();
}

}  // namespace sage

using namespace sage;

extern "C" size_t sage_k_mean_workspace_bytes(int B, int H, int N, int D) {
  const size_t S = (size_t)(N + KMEAN_ROWS - 1) / KMEAN_ROWS;
  return (size_t)B * H * S * D * sizeof(float);
}

extern "C" int sage_k_mean(const sage_tensor* k, int dtype, int B, int H, int N, int D, void* km, void* workspace,
                           sage_stream_t stream) {
  if (!tensor_ok(k, 8) || !km || !workspace || B <= 0 || H <= 0 || N <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = dim_dtype_status(D, dtype)) return s;
  const int S = kmean_chunks(N);
  float* const ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  launch_begin();
  launch_k_mean_partial(*k, B, H, N, D, dtype == SAGE_BF16, ws, S, nullptr, st);
  by_flag(dtype == SAGE_BF16, [&](auto bf) {
    hipLaunchKernelGGL((k_mean_final_kernel<decltype(bf)::value>), dim3(B * H), dim3(128), 0, st, ws, S, D, N, (uint16_t*)km);
  });
  return launch_status();
}

extern "C" int sage_quant_qk_int8(const sage_tensor* x, int dtype, int B, int H, int N, int D, const void* mean,
                                  const sage_tensor* out, float* scale, int gran, int is_key, int blk, int warp,
                                  float mult, int rounding, const void* lse_dot_vec, int dot_group, float* lse_dot,
                                  sage_stream_t stream) {
  QuantCall c;
  if (const int s = quant_check(c, x, dtype, B, H, N, D, mean, out, scale, gran, is_key, blk, warp, mult, rounding,
                                lse_dot_vec, dot_group, lse_dot))
    return s;
  return quant_launch(c, (hipStream_t)stream);
}

extern "C" int sage_quant_qk_int8_varlen(const sage_tensor* x, int dtype, const int* cu_seqlens, int num_seqs, int H,
                                         int max_seqlen, int D, const void* mean, const sage_tensor* out, float* scale,
                                         int gran, int is_key, int blk, int warp, float mult, int rounding,
                                         sage_stream_t stream) {
  if (!cu_seqlens) return SAGE_ERR_INVALID_ARGUMENT;
  QuantOptions opt;
  opt.cu = cu_seqlens;
  QuantCall c;
  if (const int s = quant_check(c, x, dtype, num_seqs, H, max_seqlen, D, mean, out, scale, gran, is_key, blk, warp, mult,
                                rounding, nullptr, 1, nullptr, opt))
    return s;
  return quant_launch(c, (hipStream_t)stream);
}

extern "C" int sage_sub_mean_f16(const sage_tensor* v, int dtype, int B, int H, int N, int D, const void* vm,
                                 const sage_tensor* out, sage_stream_t stream) {
  if (!tensor_ok(v, 8) || !tensor_ok(out, 8) || !vm || !aligned16(vm) || B <= 0 || H <= 0 || N <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = dim_dtype_status(D, dtype)) return s;
  const int RPP = 256 / (D / 8);
  const dim3 grid((N + RPP - 1) / RPP, H, B);
  launch_begin();
  by_flag(dtype == SAGE_BF16, [&](auto bf) {
    hipLaunchKernelGGL((sub_mean_f16_kernel<decltype(bf)::value>), grid, dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)v->data, v->stride_b, v->stride_h, v->stride_n, (const uint16_t*)vm,
                       (uint16_t*)out->data, out->stride_b, out->stride_h, out->stride_n, N, D);
  });
  return launch_status();
}

extern "C" int sage_quant_k_int8_kvtiles(const sage_tensor* k, int dtype, int B, int H, int N, int D, const void* mean,
                                         const sage_tensor* out, int64_t out_tile_stride, float* scale,
                                         const int64_t* scale_strides, int gran, int rounding, sage_stream_t stream) {
  if (!scale_strides || out_tile_stride <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (gran != SAGE_GRAN_PER_BLOCK && gran != SAGE_GRAN_PER_THREAD) return SAGE_ERR_INVALID_ARGUMENT;  // the K granularities
  QuantOptions opt;
  opt.out_blk_stride = out_tile_stride;
  opt.scale_strides = scale_strides;
  QuantCall c;
  if (const int s = quant_check(c, k, dtype, B, H, N, D, mean, out, scale, gran, 1, 64, 64, 1.0f, rounding, nullptr, 1, nullptr,
                                opt))
    return s;
  return quant_launch(c, (hipStream_t)stream);
}

// K smoothing + quantization as one call: km = mean over the sequence (sage_k_mean) and the INT8 quantization of k - km
// (sage_quant_qk_int8 with is_key = 1, blk 64).  Two launches at every length: the sequence is cut into at most 16 chunks
// (kmean_chunk_rows) and the quantizer finishes the mean itself; bit-identical to the two separate entry points.
extern "C" int sage_k_smooth_quant(const sage_tensor* k, int dtype, int B, int H, int N, int D, const sage_tensor* out,
                                   float* scale, void* km, int gran, int rounding, void* workspace, sage_stream_t stream) {
  KSmoothCall c;
  if (const int s = k_smooth_quant_check(c, k, dtype, B, H, N, D, out, scale, km, gran, rounding, workspace)) return s;
  return k_smooth_quant_launch(c, (hipStream_t)stream);
}

extern "C" size_t sage_kv_prepare_fp8_workspace_bytes(int B, int H, int N, int D) {
  // the fused form needs 2 x [B,H,S,D] floats; longer sequences run the separate kernels on the same buffer
  return sage_k_mean_workspace_bytes(B, H, N, D) + sage_quant_v_fp8_workspace_bytes(B, H, N, D);
}

extern "C" int sage_kv_prepare_fp8(const sage_tensor* k, const sage_tensor* v, int dtype, int B, int H, int N, int D,
                                   const sage_tensor* k_int8, float* k_scale, void* km, int gran, int rounding,
                                   const sage_tensor* v_fp8, float* v_scale, float scale_max, void* workspace,
                                   sage_stream_t stream) {
  KVPrepCall c;
  if (const int s = kv_prepare_check(c, k, v, dtype, B, H, N, D, k_int8, k_scale, km, gran, rounding, v_fp8, v_scale,
                                     scale_max, workspace))
    return s;
  return kv_prepare_launch(c, (hipStream_t)stream);
}

// ---- per-batch key lengths: the twins' arguments, then kv_lens (device, int32 [B], 4-byte aligned)
static bool kv_lens_ok(const int32_t* kv_lens) { return kv_lens && (reinterpret_cast<uintptr_t>(kv_lens) & 3u) == 0; }

extern "C" int sage_k_smooth_quant_kvlen(const sage_tensor* k, int dtype, int B, int H, int N, int D, const sage_tensor* out,
                                         float* scale, void* km, int gran, int rounding, void* workspace,
                                         const int32_t* kv_lens, sage_stream_t stream) {
  if (!kv_lens_ok(kv_lens)) return SAGE_ERR_INVALID_ARGUMENT;
  KSmoothCall c;
  if (const int s = k_smooth_quant_check(c, k, dtype, B, H, N, D, out, scale, km, gran, rounding, workspace, kv_lens)) return s;
  return k_smooth_quant_launch(c, (hipStream_t)stream);
}

extern "C" int sage_kv_prepare_fp8_kvlen(const sage_tensor* k, const sage_tensor* v, int dtype, int B, int H, int N, int D,
                                         const sage_tensor* k_int8, float* k_scale, void* km, int gran, int rounding,
                                         const sage_tensor* v_fp8, float* v_scale, float scale_max, void* workspace,
                                         const int32_t* kv_lens, sage_stream_t stream) {
  if (!kv_lens_ok(kv_lens)) return SAGE_ERR_INVALID_ARGUMENT;
  KVPrepCall c;
  if (const int s = kv_prepare_check(c, k, v, dtype, B, H, N, D, k_int8, k_scale, km, gran, rounding, v_fp8, v_scale,
                                     scale_max, workspace, kv_lens))
    return s;
  return kv_prepare_launch(c, (hipStream_t)stream);
}

// ---- persistent KV cache (include/sageattn_hip_kvcache.h): every check, the slots of the grid, one launch
// (both forms; pt: the block table of sage_kv_cache_append_paged, else null.  Paged: k, v, k_int8, k_scale and v_fp8 are the
//  pools, P their page count, N the logical capacity; the quantizer's parameters are those of one page of page_size rows)
static int kv_cache_append(const sage_tensor* k, const sage_tensor* v, int dtype, int B, int H, int N, int D, const void* km,
                           const sage_tensor* k_int8, float* k_scale, int gran, int rounding, const sage_tensor* v_fp8,
                           const float* v_coef, const int32_t* start_lens, const int32_t* kv_lens, int max_new,
                           const KvPageTable* pt, int P, sage_stream_t stream) {
  if (!km || !aligned16(km) || !kv_lens_ok(start_lens) || !kv_lens_ok(kv_lens) || max_new < 1) return SAGE_ERR_INVALID_ARGUMENT;
  if (v_fp8 && (!v_coef || !aligned16(v_coef) || !tensor_ok(v, 8) || !tensor_ok(v_fp8, 16))) return SAGE_ERR_INVALID_ARGUMENT;
  if (gran != SAGE_GRAN_PER_BLOCK && gran != SAGE_GRAN_PER_THREAD) return SAGE_ERR_INVALID_ARGUMENT;  // the K granularities
  if (B <= 0 || N <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  QuantCall c;
  if (const int s = quant_check(c, k, dtype, pt ? P : B, H, pt ? 64 << pt->shift : N, D, km, k_int8, k_scale, gran, 1, 64, 64,
                                1.0f, rounding, nullptr, 1, nullptr))
    return s;
  c.p.N = N;
  KvAppendParams a;
  a.k = c.p;
  a.v = VPrepParams();
  a.v_coef = v_coef;
  if (v_fp8) {
    a.v.v = (const uint16_t*)v->data; a.v.sb = v->stride_b; a.v.sh = v->stride_h; a.v.sn = v->stride_n;
    a.v.out = (uint8_t*)v_fp8->data; a.v.ob = v_fp8->stride_b; a.v.oh = v_fp8->stride_h; a.v.od = v_fp8->stride_n; a.v.o_tile = 64;
  }
  a.start_lens = start_lens;
  a.kv_lens = kv_lens;
  // K slots: the tile that holds row min(start_b, len_b - 1), then the tiles of at most max_new further rows
  const int ntile = (N + 63) / 64;
  const int k_slots = std::min((std::min(max_new, N) + 63) / 64 + 1, ntile);
  a.k_slots = k_slots;
  // V slots: k_slots consecutive tiles lie in at most k_slots / blks + 1 units of blks tiles (blks == 1: in k_slots)
  const int blks = by_dim(D, [](auto d) { return VQuantGeom<decltype(d)::value>::BLKS; });
  const int v_slots = !v_fp8 ? 0 : blks == 1 ? k_slots : std::min(k_slots / blks + 1, (ntile + blks - 1) / blks);
  launch_begin();
  by_dim(D, [&](auto d) {
    by_flag(c.bf16, [&](auto bf) {
      by_flag(rounding == SAGE_ROUND_TRITON, [&](auto tr) {
        by_flag(v_fp8 != nullptr, [&](auto wv) {
          if (pt)
            hipLaunchKernelGGL((kv_cache_append_paged_kernel<decltype(d)::value, decltype(bf)::value, decltype(tr)::value,
                                                             decltype(wv)::value>),
                               dim3(k_slots + v_slots, H, B), dim3(256), 0, (hipStream_t)stream, a, *pt);
          else
          hipLaunchKernelGGL((kv_cache_append_kernel<decltype(d)::value, decltype(bf)::value, decltype(tr)::value,
                                                     decltype(wv)::value>),
                             dim3(k_slots + v_slots, H, B), dim3(256), 0, (hipStream_t)stream, a);
        });
      });
    });
  });
  return launch_status();
}

extern "C" int sage_kv_cache_append(const sage_tensor* k, const sage_tensor* v, int dtype, int B, int H, int N, int D,
                                    const void* km, const sage_tensor* k_int8, float* k_scale, int gran, int rounding,
                                    const sage_tensor* v_fp8, const float* v_coef, const int32_t* start_lens,
                                    const int32_t* kv_lens, int max_new, sage_stream_t stream) {
  return kv_cache_append(k, v, dtype, B, H, N, D, km, k_int8, k_scale, gran, rounding, v_fp8, v_coef, start_lens, kv_lens,
                         max_new, nullptr, 0, stream);
}

// ---- paged KV cache (include/sageattn_hip_paged.h): the table's own arguments, then the checks and the launch above
extern "C" int sage_kv_cache_append_paged(const sage_tensor* k_pool, const sage_tensor* v_pool, int dtype, int B, int H, int D,
                                          const void* km, const sage_tensor* k8_pool, float* k_scale_pool, int gran,
                                          int rounding, const sage_tensor* v8_pool, const float* v_coef,
                                          const int32_t* block_table, int64_t table_stride, int max_pages, int page_size,
                                          int num_pages, const int32_t* start_lens, const int32_t* kv_lens, int max_new,
                                          sage_stream_t stream) {
  if (page_size != 64 && page_size != 128 && page_size != 256) return SAGE_ERR_INVALID_ARGUMENT;
  if (!kv_lens_ok(block_table) || max_pages < 1 || num_pages < 1 || table_stride < max_pages) return SAGE_ERR_INVALID_ARGUMENT;
  if ((int64_t)max_pages * page_size > INT_MAX) return SAGE_ERR_TOO_LARGE;
  KvPageTable pt;
  pt.table = block_table;
  pt.stride = table_stride;
  pt.shift = page_size == 64 ? 0 : page_size == 128 ? 1 : 2;
  return kv_cache_append(k_pool, v_pool, dtype, B, H, max_pages * page_size, D, km, k8_pool, k_scale_pool, gran, rounding,
                         v8_pool, v_coef, start_lens, kv_lens, max_new, &pt, num_pages, stream);
}

// ---- paged KV cache without fp16 pools (include/sageattn_hip_paged_rows.h): every check, then one launch
extern "C" int sage_kv_cache_append_rows_paged(const sage_tensor* k_new, const sage_tensor* v_new, int dtype, int B, int H, int T,
                                               int D, const void* km, void* k_tail, const sage_tensor* k8_pool,
                                               float* k_scale_pool, int gran, int rounding, const sage_tensor* v_pool,
                                               const sage_tensor* v8_pool, const float* v_coef, const int32_t* block_table,
                                               int64_t table_stride, int max_pages, int page_size, int num_pages,
                                               const int32_t* start_lens, const int32_t* kv_lens, sage_stream_t stream) {
  if (page_size != 64 && page_size != 128 && page_size != 256) return SAGE_ERR_INVALID_ARGUMENT;
  if (!kv_lens_ok(block_table) || max_pages < 1 || num_pages < 1 || table_stride < max_pages) return SAGE_ERR_INVALID_ARGUMENT;
  if ((int64_t)max_pages * page_size > INT_MAX) return SAGE_ERR_TOO_LARGE;
  if (!km || !aligned16(km) || !kv_lens_ok(start_lens) || !kv_lens_ok(kv_lens) || T < 1) return SAGE_ERR_INVALID_ARGUMENT;
  if (!k_tail || !aligned16(k_tail) || (v_pool != nullptr) == (v8_pool != nullptr)) return SAGE_ERR_INVALID_ARGUMENT;
  if (!tensor_ok(v_new, 8) || (v_pool && !tensor_ok(v_pool, 8))) return SAGE_ERR_INVALID_ARGUMENT;
  if (v8_pool && (!v_coef || !aligned16(v_coef) || !tensor_ok(v8_pool, 16))) return SAGE_ERR_INVALID_ARGUMENT;
  if (gran != SAGE_GRAN_PER_BLOCK && gran != SAGE_GRAN_PER_THREAD) return SAGE_ERR_INVALID_ARGUMENT;  // the K granularities
  if (B <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  QuantCall c;  // (x = k_new stands for the rows: the parameters are those of one page of page_size rows, as the paged append's)
  if (const int s = quant_check(c, k_new, dtype, num_pages, H, page_size, D, km, k8_pool, k_scale_pool, gran, 1, 64, 64, 1.0f,
                                rounding, nullptr, 1, nullptr))
    return s;
  // the bytes inside one (page, head) slice stay below 2^31, as the attention kernels need them
  const int64_t lim = (int64_t)1 << 31;
  if ((int64_t)page_size * k8_pool->stride_n + D >= lim) return SAGE_ERR_TOO_LARGE;
  if (v_pool && ((int64_t)page_size * v_pool->stride_n + D) * 2 >= lim) return SAGE_ERR_TOO_LARGE;
  if (v8_pool && (int64_t)D * v8_pool->stride_n + page_size >= lim) return SAGE_ERR_TOO_LARGE;
  const int N = max_pages * page_size;
  c.p.N = N;
  KvAppendParams a;
  a.k = c.p;
  a.v = VPrepParams();
  a.v_coef = v_coef;
  if (v8_pool) {
    a.v.out = (uint8_t*)v8_pool->data; a.v.ob = v8_pool->stride_b; a.v.oh = v8_pool->stride_h; a.v.od = v8_pool->stride_n; a.v.o_tile = 64;
  }
  a.start_lens = start_lens;
  a.kv_lens = kv_lens;
  KvPageTable pt;
  pt.table = block_table;
  pt.stride = table_stride;
  pt.shift = page_size == 64 ? 0 : page_size == 128 ? 1 : 2;
  KvRowsParams r;
  r.k_new = (const uint16_t*)k_new->data; r.ksb = k_new->stride_b; r.ksh = k_new->stride_h; r.ksn = k_new->stride_n;
  r.v_new = (const uint16_t*)v_new->data; r.vsb = v_new->stride_b; r.vsh = v_new->stride_h; r.vsn = v_new->stride_n;
  r.k_tail = (uint16_t*)k_tail;
  r.v_pool = v_pool ? (uint16_t*)v_pool->data : nullptr;
  r.vpb = v_pool ? v_pool->stride_b : 0; r.vph = v_pool ? v_pool->stride_h : 0; r.vpn = v_pool ? v_pool->stride_n : 0;
  r.T = T;
  // the slots of sage_kv_cache_append_paged with max_new = T (FP16 / BF16 P.V: the V units copy rows)
  const int ntile = (N + 63) / 64;
  const int k_slots = std::min((std::min(T, N) + 63) / 64 + 1, ntile);
  a.k_slots = k_slots;
  const int blks = by_dim(D, [](auto d) { return VQuantGeom<decltype(d)::value>::BLKS; });
  const int v_slots = blks == 1 ? k_slots : std::min(k_slots / blks + 1, (ntile + blks - 1) / blks);
  launch_begin();
  by_dim(D, [&](auto d) {
    by_flag(c.bf16, [&](auto bf) {
      by_flag(rounding == SAGE_ROUND_TRITON, [&](auto tr) {
        by_flag(v8_pool != nullptr, [&](auto f8) {
          hipLaunchKernelGGL((kv_cache_append_rows_paged_kernel<decltype(d)::value, decltype(bf)::value, decltype(tr)::value,
                                                                decltype(f8)::value ? 1 : 0>),
                             dim3(k_slots + v_slots, H, B), dim3(256), 0, (hipStream_t)stream, a, pt, r);
        });
      });
    });
  });
  return launch_status();
}
