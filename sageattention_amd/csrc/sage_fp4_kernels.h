// The MXFP4 V quantizer (include/sageattn_hip_fp4.h holds the rule) as a device function: one UNIT -- the 64-token tiles a
// workgroup of 256 threads covers, one at head_dim 128 and two at 64 (VQuantGeom) -- of one (b, kv head), shared by the
// stand-alone kernel (sage_fp4.hip) and by the cache append (sage_quant.hip, kv_cache_append_v4_kernel); and its paged form.
//
// One pass, no statistics launch: the scale groups live inside a tile.  A thread owns 8 channels of FOUR consecutive tokens
// (the geometry and the clamped, unconditional row loads of the FP8 quantizer, sage_fp8_kernels.h).  In the order of the
// image the four tokens 4g .. 4g+3 are four consecutive elements of ONE lane half hh = g / 8: four nibbles, one 16-bit word
// per channel.  The 32 tokens of a group G(t, c, hh) belong to the 8 threads of a channel run with the token groups 8 hh ..
// 8 hh + 7, so the group maximum is 8 partial maxima out of LDS -- deterministic, no atomics.  The [d][32-byte] image and
// the 2 * D scale bytes of the tile are staged in LDS and leave as 16-byte stores.
#pragma once
#include "sage_fp8_kernels.h"

namespace sage {

// the caller's image and scale tensors: uint8 [B,H,D,32*T] (od = stride of a channel) and uint8 [B,H,T,2*D]
struct V4Image {
  uint8_t* img;
  int64_t ob, oh, od;
  uint8_t* scale;
  int64_t sb, sh;  // bytes per batch and per head; a tile's 2 * D bytes are contiguous, tiles 2 * D apart
};

// LDS of a unit, in dwords: the partial maxima [token group][D], then per tile the image (D rows of 32 bytes, a row of 8
// dwords padded to 9: the 16-bit stores of the 8 threads of a token group then spread over the banks) and the scale bytes
template <int D>
struct V4QuantGeom {
  using G = VQuantGeom<D>;
  static constexpr int PM = G::TG * D;          // partial maxima
  static constexpr int ROW = 9;                 // dwords per image row in LDS
  static constexpr int IMG = D * ROW;           // image of a tile
  static constexpr int SC = 2 * D / 4;          // scale bytes of a tile
  static constexpr int LDS = PM + G::BLKS * (IMG + SC);
};

// e8m0 byte of a group maximum a >= 0 (finite): the smallest power of two 2^(E-127) with a <= 6 * 2^(E-127), from the bits
// of the float: a = m * 2^e, 1 <= m < 2, is at most 1.5 * 2^(k+2) iff k + 2 >= e + (m > 1.5).  Zero: 127.
__device__ __forceinline__ int mxfp4_scale_byte(const float a) {
  const uint32_t u = __float_as_uint(a);
  const int e = (int)(u >> 23) - 2 + ((u & 0x7fffffu) > 0x400000u ? 1 : 0);
  return u == 0u ? 127 : min(max(e, 0), 254);
}
// e2m1 code (sign in bit 3) of y = v * 2^(127-E): nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the even code, saturating.
// The grid has steps 0.5 below 2, 1 below 4 and 2 above; rintf is round-to-nearest-even and the codes count the grid points,
// so an even rintf result is an even code in each of the three ranges.
__device__ __forceinline__ uint32_t e2m1_code(const float y) {
  const float m = fabsf(y);
  const float c = m < 2.f ? rintf(m * 2.f) : m < 4.f ? rintf(m) + 2.f : fminf(rintf(m * 0.5f) + 4.f, 7.f);
  return (uint32_t)(int)c | ((__float_as_uint(y) >> 28) & 8u);
}

// Unit `unit` of (b, h) at length len > 0: quantize its tiles below ceil(len / 64) and store those at or above tile `t_lo`
// (the stand-alone quantizer: 0; the append: its first touched tile, so that no byte of another tile is written).  Rows at and
// beyond len are never loaded; their nibbles are 0 and a group without a valid row has the scale byte 127.  Contains two
// barriers: every thread of the workgroup must call it.
template <int D, bool BF16>
__device__ __forceinline__ void v4_quant_unit(const uint16_t* __restrict__ v, const int64_t sb, const int64_t sh, const int64_t sn,
                                              const int len, const V4Image& o, const int unit, const int t_lo, const int h,
                                              const int b, uint32_t* __restrict__ lds) {
  using G = VQuantGeom<D>;
  using L = V4QuantGeom<D>;
  constexpr int TPR = G::TPR;
  uint4 raw[4];
  v_quant_load<D>(v + b * sb + h * sh, sn, len, unit, raw);
  const int tid = threadIdx.x;
  const int tg = tid / TPR, tc = tid % TPR;
  const int bi = tg / 16, g16 = tg % 16, t0 = 4 * g16;
  const int blk = unit * G::BLKS + bi;
  float x[4][8], amax[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) amax[j] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool valid = blk * 64 + t0 + i < len;
    float f[8];
    unpack8<BF16>(raw[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[i][j] = valid ? f[j] : 0.f;
      amax[j] = fmaxf(amax[j], fabsf(x[i][j]));
    }
  }
  float* const pm = reinterpret_cast<float*>(lds);
  *reinterpret_cast<float4*>(pm + tg * D + tc * 8) = make_float4(amax[0], amax[1], amax[2], amax[3]);
  *reinterpret_cast<float4*>(pm + tg * D + tc * 8 + 4) = make_float4(amax[4], amax[5], amax[6], amax[7]);
  __syncthreads();
  // the group of the thread's tokens: lane half hh = the half of the tile they lie in
  const int hh = g16 >> 3;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const float* src = pm + (bi * 16 + 8 * hh + m) * D + tc * 8;
    const float4 a = *reinterpret_cast<const float4*>(src), c = *reinterpret_cast<const float4*>(src + 4);
    amax[0] = fmaxf(amax[0], a.x); amax[1] = fmaxf(amax[1], a.y); amax[2] = fmaxf(amax[2], a.z); amax[3] = fmaxf(amax[3], a.w);
    amax[4] = fmaxf(amax[4], c.x); amax[5] = fmaxf(amax[5], c.y); amax[6] = fmaxf(amax[6], c.z); amax[7] = fmaxf(amax[7], c.w);
  }
  // token 32*hh + w is element (w&3) + 4*(w>>3) + 16*((w>>2)&1) of lane half hh (the header derives it): the thread's four
  // tokens are the elements 16*((w0>>2)&1) + 4*(w0>>3) + 0..3, i.e. the 16-bit word 8*hh + 4*((w0>>2)&1) + (w0>>3) of the
  // channel's 32-byte row, element 0 in the low nibble of the first byte
  const int w0 = t0 & 31;
  const int half_word = 8 * hh + 4 * ((w0 >> 2) & 1) + (w0 >> 3);  // index of the 16-bit word in the row
  uint16_t* const img16 = reinterpret_cast<uint16_t*>(lds + L::PM + bi * (L::IMG + L::SC));
  uint8_t* const sc8 = reinterpret_cast<uint8_t*>(lds + L::PM + bi * (L::IMG + L::SC) + L::IMG);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int d = tc * 8 + j;
    const int E = mxfp4_scale_byte(amax[j]);
    const float inv = __uint_as_float((uint32_t)(254 - E) << 23);  // 2^(127-E): E <= 253 for a finite maximum
    const uint32_t w = e2m1_code(x[0][j] * inv) | (e2m1_code(x[1][j] * inv) << 4) | (e2m1_code(x[2][j] * inv) << 8) |
                       (e2m1_code(x[3][j] * inv) << 12);
    img16[d * (2 * L::ROW) + half_word] = (uint16_t)w;
    // the scale bytes of a tile: [hh][c % 32][c / 32] -- lane (r, hh) of the attention kernel finds the bytes of its channels
    // r, r + 32, ... side by side, one load per tile
    if ((g16 & 7) == 0) sc8[(hh * 32 + (d & 31)) * (D / 32) + (d >> 5)] = (uint8_t)E;
  }
  __syncthreads();
  const int ntile = (len + 63) >> 6;
  for (int c = tid; c < G::BLKS * D * 2; c += 256) {
    const int bo = c / (D * 2), cc = c % (D * 2), d = cc >> 1, ch = cc & 1;
    const int ob_blk = unit * G::BLKS + bo;
    if (ob_blk >= ntile || ob_blk < t_lo) continue;
    const uint32_t* s = lds + L::PM + bo * (L::IMG + L::SC) + d * L::ROW + ch * 4;
    *reinterpret_cast<uint4*>(o.img + b * o.ob + h * o.oh + (int64_t)d * o.od + (int64_t)ob_blk * 32 + ch * 16) =
        make_uint4(s[0], s[1], s[2], s[3]);
  }
  for (int c = tid; c < G::BLKS * (2 * D / 16); c += 256) {
    const int bo = c / (2 * D / 16), ch = c % (2 * D / 16);
    const int ob_blk = unit * G::BLKS + bo;
    if (ob_blk >= ntile || ob_blk < t_lo) continue;
    const uint32_t* s = lds + L::PM + bo * (L::IMG + L::SC) + L::IMG + ch * 4;
    *reinterpret_cast<uint4*>(o.scale + b * o.sb + h * o.sh + (int64_t)ob_blk * (2 * D) + ch * 16) = make_uint4(s[0], s[1], s[2], s[3]);
  }
}

// The unit of a PAGED cache (include/sageattn_hip_paged_fp4.h; the append of sage_quant.hip): v4_quant_unit with the rows and
// the tiles looked up per 64-token block.  `v` and `o` are POOLS -- sb, o.ob and o.sb the strides of a page, the image
// [P,H,D,32*tpp], the scale bytes [P,H,tpp,2*D] -- a page holds 1 << shift tiles and page_of(blk) is the page of logical tile
// blk of this sequence.  At head_dim 64 a unit is two blocks, which with 64-key pages lie in two pages: the two halves of the
// workgroup look up their own.  A row index clamped to len - 1 (the loads are unconditional, as in v_quant_load) lies in block
// min(blk, ntile - 1): a block the sequence has, whose page is named; a tile below t_lo or at or beyond ceil(len / 64) is not
// stored and its page is not asked for.  The arithmetic between the loads and the stores is v4_quant_unit's, statement for
// statement (a text of its own: with the middle shared through one function, the head_dim-64 instantiations of
// v_quant_mxfp4_kernel and all of kv_cache_append_v4_kernel came out with other instruction streams).
template <int D, bool BF16, class PageOf>
__device__ __forceinline__ void v4_quant_unit_paged(const uint16_t* __restrict__ v, const int64_t sb, const int64_t sh,
                                                    const int64_t sn, const int len, const V4Image& o, const int shift,
                                                    const PageOf page_of, const int unit, const int t_lo, const int h,
                                                    uint32_t* __restrict__ lds) {
  using G = VQuantGeom<D>;
  using L = V4QuantGeom<D>;
  constexpr int TPR = G::TPR;
  const int tid = threadIdx.x;
  const int tg = tid / TPR, tc = tid % TPR;
  const int bi = tg / 16, g16 = tg % 16, t0 = 4 * g16;
  const int blk = unit * G::BLKS + bi;
  const int tmask = (1 << shift) - 1, ntile = (len + 63) >> 6;
  uint4 raw[4];
  {
    const int blk_c = min(blk, ntile - 1);
    const uint16_t* vbase = v + page_of(blk_c) * sb + h * sh + (int64_t)((blk_c & tmask) * 64) * sn + tc * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) raw[i] = *reinterpret_cast<const uint4*>(vbase + (int64_t)(min(blk * 64 + t0 + i, len - 1) & 63) * sn);
  }
  float x[4][8], amax[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) amax[j] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool valid = blk * 64 + t0 + i < len;
    float f[8];
    unpack8<BF16>(raw[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[i][j] = valid ? f[j] : 0.f;
      amax[j] = fmaxf(amax[j], fabsf(x[i][j]));
    }
  }
  float* const pm = reinterpret_cast<float*>(lds);
  *reinterpret_cast<float4*>(pm + tg * D + tc * 8) = make_float4(amax[0], amax[1], amax[2], amax[3]);
  *reinterpret_cast<float4*>(pm + tg * D + tc * 8 + 4) = make_float4(amax[4], amax[5], amax[6], amax[7]);
  __syncthreads();
  const int hh = g16 >> 3;  // the group of the thread's tokens: the half of the tile they lie in
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const float* src = pm + (bi * 16 + 8 * hh + m) * D + tc * 8;
    const float4 a = *reinterpret_cast<const float4*>(src), c = *reinterpret_cast<const float4*>(src + 4);
    amax[0] = fmaxf(amax[0], a.x); amax[1] = fmaxf(amax[1], a.y); amax[2] = fmaxf(amax[2], a.z); amax[3] = fmaxf(amax[3], a.w);
    amax[4] = fmaxf(amax[4], c.x); amax[5] = fmaxf(amax[5], c.y); amax[6] = fmaxf(amax[6], c.z); amax[7] = fmaxf(amax[7], c.w);
  }
  const int w0 = t0 & 31;
  const int half_word = 8 * hh + 4 * ((w0 >> 2) & 1) + (w0 >> 3);  // index of the 16-bit word in the row (v4_quant_unit)
  uint16_t* const img16 = reinterpret_cast<uint16_t*>(lds + L::PM + bi * (L::IMG + L::SC));
  uint8_t* const sc8 = reinterpret_cast<uint8_t*>(lds + L::PM + bi * (L::IMG + L::SC) + L::IMG);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int d = tc * 8 + j;
    const int E = mxfp4_scale_byte(amax[j]);
    const float inv = __uint_as_float((uint32_t)(254 - E) << 23);  // 2^(127-E): E <= 253 for a finite maximum
    const uint32_t w = e2m1_code(x[0][j] * inv) | (e2m1_code(x[1][j] * inv) << 4) | (e2m1_code(x[2][j] * inv) << 8) |
                       (e2m1_code(x[3][j] * inv) << 12);
    img16[d * (2 * L::ROW) + half_word] = (uint16_t)w;
    if ((g16 & 7) == 0) sc8[(hh * 32 + (d & 31)) * (D / 32) + (d >> 5)] = (uint8_t)E;
  }
  __syncthreads();
  for (int c = tid; c < G::BLKS * D * 2; c += 256) {
    const int bo = c / (D * 2), cc = c % (D * 2), d = cc >> 1, ch = cc & 1;
    const int ob_blk = unit * G::BLKS + bo;
    if (ob_blk >= ntile || ob_blk < t_lo) continue;
    const uint32_t* s = lds + L::PM + bo * (L::IMG + L::SC) + d * L::ROW + ch * 4;
    *reinterpret_cast<uint4*>(o.img + page_of(ob_blk) * o.ob + h * o.oh + (int64_t)d * o.od + (ob_blk & tmask) * 32 + ch * 16) =
        make_uint4(s[0], s[1], s[2], s[3]);
  }
  for (int c = tid; c < G::BLKS * (2 * D / 16); c += 256) {
    const int bo = c / (2 * D / 16), ch = c % (2 * D / 16);
    const int ob_blk = unit * G::BLKS + bo;
    if (ob_blk >= ntile || ob_blk < t_lo) continue;
    const uint32_t* s = lds + L::PM + bo * (L::IMG + L::SC) + L::IMG + ch * 4;
    *reinterpret_cast<uint4*>(o.scale + page_of(ob_blk) * o.sb + h * o.sh + (ob_blk & tmask) * (2 * D) + ch * 16) =
        make_uint4(s[0], s[1], s[2], s[3]);
  }
}

}  // namespace sage
