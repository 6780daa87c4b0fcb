/*
 * sageattn_hip_fp4.h -- extension of the C ABI (sageattn_hip.h, sageattn_hip_kvcache.h): an MXFP4 image of V for the
 * persistent quantized KV cache of the split-KV attention entry points.  Same conventions: device pointers, element strides,
 * the caller owns every buffer, every argument is checked before the launch and a call that returns an argument status has
 * enqueued nothing.
 *
 * Few query rows against a long cache are bound by the bytes of K and V, and V is the larger half: 256 bytes per key and KV
 * head in fp16 at head_dim 128, 128 in FP8.  The P.V product of the FP8 form runs on v_mfma_scale_f32_32x32x64_f8f6f4, which
 * takes its two operands in different formats: here A = V^T is FP4 (e2m1) with one e8m0 block scale per 32 tokens of a
 * channel, 64 + 4 bytes per key, and B = P stays e4m3.  The K half (k8, k_scale, km) is that of sageattn_hip_kvcache.h,
 * by the same rule and the same code.
 *
 * THE V IMAGE
 *
 * Shapes, per (b, kv head) and 64-key tile t, T = ceil(N / 64):
 *   img    uint8 [B,H,D,32*T]: img[b,h,c,32*t + i], two e2m1 nibbles per byte
 *   scale  uint8 [B,H,T,2*D], contiguous: e8m0 bytes, value 2^(byte - 127)
 *
 * Token order.  Inside a tile the tokens stand so that P^T is the S^T accumulators as they are, as in the FP8 image -- but
 * not in the FP8 image's order, because the instruction numbers the K index of a 4-bit and of an 8-bit operand differently.
 * The e4m3 B operand holds K index 32*(i >> 4) + 16*h + (i & 15) in byte i of lane half h, and byte i = 16*mt + reg of P^T is
 * key 32*mt + (reg & 3) + 8*(reg >> 2) + 4*h.  The e2m1 A operand holds K index 32*hh + j in nibble j of lane half hh.  Equal
 * K indices meet, so lane half hh (0 / 1) of the A fragment holds, as 32 consecutive nibbles, the tokens
 *   kv(hh, j) = 32*hh + (j & 3) + 8*((j & 15) >> 2) + 4*(j >> 4),   j = 0 .. 31.
 * Element j of half hh is nibble (j & 1) -- 0 = bits 3:0, as the instruction reads its operand -- of byte 16*hh + (j >> 1) of
 * the channel's 32 bytes of the tile.  A scale group G(t, c, hh) is therefore the tokens 32*hh .. 32*hh + 31 of tile t: one
 * lane's 32 values, which is what one scale byte of the instruction covers.  A nibble is sign (bit 3), two exponent bits, one mantissa bit: the codes 0 .. 7 are
 * 0, .5, 1, 1.5, 2, 3, 4, 6.  The layout is private to this library, as the FP8 one is.
 *
 * Scale bytes.  The 2*D bytes of a tile are ordered [hh][c % 32][c / 32]: byte (hh*32 + c % 32) * (D/32) + c / 32 is the
 * scale of G(t, c, hh).  Lane (r, hh) of the attention kernel owns the channels r, r + 32, ...: their D/32 bytes are one
 * aligned load per tile (a dword at head_dim 128), and the MFMA of channel block dt selects byte dt.
 *
 * Quantization of a group, over its rows < len_b only (len_b = clamp(kv_lens[b], 0, N), N without kv_lens); rows at or
 * beyond len_b are never loaded, NaN there changes nothing:
 *   1. a = max |v| over the valid rows.
 *   2. no valid row, or a == 0: scale byte 127, nibbles 0.
 *   3. else the byte E = clamp(127 + ceil(log2(a / 6)), 0, 254): the smallest power of two under which nothing saturates,
 *      computed exactly from the bits of a.
 *   4. a valid element is v * 2^(127-E) rounded to the nearest e2m1 value, ties to the even code, saturating at +-6.
 *   5. elements of invalid rows are 0.
 * The byte 0xFF (e8m0 NaN) is never written.  Inf / NaN in valid rows is outside the contract, as for INT8 K.  Of batch b
 * the tiles below ceil(len_b / 64) are written, the ragged one with its zero nibbles and 127 bytes; no byte of a tile at or
 * beyond it.
 *
 * GROWTH.  A scale group lies inside one tile, like the scale groups of K, so growth is local and nothing is frozen: there
 * are no V coefficients and no headroom.  sage_kv_cache_append_v4 brings K (the rule of sageattn_hip_kvcache.h, the same
 * tile body) and the image up to date in ONE launch: with start_b and len_b as there, it touches the tiles
 * t0_b .. ceil(len_b / 64) - 1, t0_b = floor(min(start_b, len_b - 1) / 64); every touched tile of the image and of the scales
 * is bit-identical to sage_quant_v_mxfp4(v[b, :, :len_b]); no row >= len_b is loaded and no byte of another tile is
 * written; start_b >= len_b re-quantizes exactly the ragged tile; len_b == 0 touches nothing.  The preconditions (rows below
 * start_b unchanged, len_b - min(start_b, len_b) <= max_new) are those of sage_kv_cache_append.
 *
 * ATTENTION.  sage_attn_fusedq_pv_f4_splitkv[_causal] are sage_attn_fusedq_pv_f8_splitkv[_causal] with the image and its
 * scale bytes in the place of v_fp8 and v_scale: the same split rule, workspace (sage_splitkv_workspace_bytes), merge, key
 * lengths, causal alignment and q_fold, and the same arithmetic for P, the row sums and the LSE in the same order -- lse is
 * bit-identical to the FP8 form's on the same K operands.  There is no per-channel V scale in the epilogue.
 *
 * The image for a cache kept in pages: sageattn_hip_paged_fp4.h.
 *
 * NOT BUILT: an FP4 image for the paged cache without fp16 pools (sageattn_hip_paged_rows.h: it would need an fp16 V tail per
 * sequence) and the shared-prefix operator on the paged FP4 cache; the uncached and dense operators (their pre-pass reads
 * fp16 V: no bytes are saved); FP4 / FP6 for P or for Q / K (which would also double the MFMA rate); V smoothing.
 */
#ifndef SAGEATTN_HIP_FP4_H
#define SAGEATTN_HIP_FP4_H

#include "sageattn_hip_kvcache.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Quantize v [B,H,N,D] (fp16 / bf16, dtype) to the image by the rule above, in one launch and one pass over v.
 *   img     its data, 16-byte aligned; stride_n = the stride of a channel d (bytes), stride_b / stride_h those of batch and
 *           head, all multiples of 16; the 32 bytes of tile t of a channel start at 32*t
 *   scale   uint8 [B,H,T,2*D] contiguous, 16-byte aligned
 *   kv_lens int32 [B] on the device, 4-byte aligned, or NULL: every batch has N rows
 * A NULL or misaligned pointer, B, H or N < 1, an unknown dtype -> SAGE_ERR_INVALID_ARGUMENT; D not 64 or 128 ->
 * SAGE_ERR_UNSUPPORTED_HEAD_DIM. */
int sage_quant_v_mxfp4(const sage_tensor* v, int dtype, int B, int H, int N, int D, const sage_tensor* img, uint8_t* scale,
                       const int32_t* kv_lens, sage_stream_t stream);

/* sage_kv_cache_append with the MXFP4 image as its V half: (K tile slots + V unit slots, H, B) workgroups, one launch.  The
 * K arguments and their checks are those of sage_kv_cache_append; v, img and scale as above, all required. */
int sage_kv_cache_append_v4(const sage_tensor* k, const sage_tensor* v, int dtype, int B, int H, int N, int D, const void* km,
                            const sage_tensor* k_int8, float* k_scale, int gran, int rounding, const sage_tensor* img,
                            uint8_t* scale, const int32_t* start_lens, const int32_t* kv_lens, int max_new,
                            sage_stream_t stream);

/* Split-KV attention on the image: the arguments, checks and statuses of sage_attn_fusedq_pv_f8_splitkv[_causal], with
 * v_img / v_img_scale in the place of v_fp8 / v_scale (NULL or misaligned: SAGE_ERR_INVALID_ARGUMENT; a (b, head) slice
 * beyond the 32-bit window: SAGE_ERR_TOO_LARGE) and no v_mean. */
int sage_attn_fusedq_pv_f4_splitkv(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_img,
                                   const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                   const uint8_t* v_img_scale, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                   int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens, int num_splits,
                                   void* workspace, size_t workspace_bytes, sage_stream_t stream);
int sage_attn_fusedq_pv_f4_splitkv_causal(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_img,
                                          const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                          const uint8_t* v_img_scale, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                          int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens, int num_splits,
                                          int q_fold, void* workspace, size_t workspace_bytes, sage_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGEATTN_HIP_FP4_H */
