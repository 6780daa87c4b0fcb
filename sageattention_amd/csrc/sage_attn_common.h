// Device helpers and the kernel parameter block of the attention kernel (sage_attn.hip).
#pragma once
#include <type_traits>
#include "sage_common.h"

namespace sage {

struct AttnParams {
  const int8_t* q; int64_t qsb, qsh, qsn;
  const int8_t* k; int64_t ksb, ksh, ksn;
  const uint8_t* v; int64_t vsb, vsh, vsn;  // byte pointer; strides in ELEMENTS of v's dtype
  uint16_t* o; int64_t osb, osh, osn;
  const float* q_scale; const float* k_scale; const float* v_scale; const float* v_mean;
  float* lse;
  int B, Hq, Hk, M, N;
  int nqb;      // query blocks per (b,h)
  int gq, gk;   // scales per (b,h)
  int qgran, blkq, warpq;
  float logit_mult;
  int out_bf16;
  // varlen (packed sequences, core.py:363-477): when cu_q/cu_k are set, "batch" b is sequence b, its rows are
  // [cu[b], cu[b+1]) of the packed [total, H, D] tensors (stride_b unused) and p.M / p.N are the maximum lengths
  // (per-batch key lengths -- attn_i8_kvlen_kernel, sage_attn_kvlen.hip -- have no packed form: kv_lens, int32 [B], shares
  //  the word of cu_k, which the other kernels read only behind a non-null cu_q)
  const int* cu_q;
  union { const int* cu_k; const int32_t* kv_lens; };
  // fused Q quantizer: when q_f16 is set, q/q_scale are ignored and every wave quantizes its own 32 query rows in the
  // prologue (per_warp: CUDA numerics, per_thread: Triton numerics -- the pairings of core.py:621-624); km (optional,
  // [B,Hk,D] in q's dtype) yields the LSE correction q.km and lse then receives the FINAL natural-log LSE (core.py:651)
  const uint16_t* q_f16;
  const uint16_t* km;
  int q_bf16;
  float sm_scale;
  // attn_mask of sageattn_qk_int8_pv_fp16_triton (core.py:306-318; kernels attn_qk_int8_per_block.py:33-52):
  // [B,H,M,N] view with element strides (0 = broadcast); kind 1 = bool (False -> -1e6), 2 = fp16, 3 = bf16 (added to
  // the base-2 logits, exactly as the reference adds it after its sm_scale*log2e scaling)
  // (block-sparse attention has no attn_mask form: its list descriptor shares the two words, so the parameter block of the
  //  dense kernels keeps its size and layout)
  // bs_lists / bs_row: the tile lists of sage_block_map_compact, one row of bs_row int32 per (b, h_q, 128-row q-block):
  // [count, tile_0 < tile_1 < ..., kBlockListPad copies of the last tile]
  // (split-KV attention -- attn_i8_splitkv_kernel, sage_attn_splitkv.hip -- has neither an attn_mask nor lists: its workspace
  //  shares these words as well.  sk_o fp32 [S,B,Hq,M,D], the normalised partial outputs; sk_lse fp32 [S,B,Hq,M], their raw
  //  base-2 LSEs; num_splits = S.  Its optional kv_lens is the word of cu_k above, null = every batch has N keys)
  union { const uint8_t* mask; const int* bs_lists; float* sk_o; };
  // (the P.V skip of the block-sparse form -- attn_i8_blocksparse_pvskip_kernel -- keeps its two pointers in the first two
  //  mask strides: pv_thresh fp32 [Hq], pv_skipped int32 [B,Hq,nqb,4] or null)
  union { int64_t msb; const float* pv_thresh; float* sk_lse; };
  // (paged split-KV -- attn_i8_splitkv_paged_kernel / attn_i8_splitkv_causal_paged_kernel, include/sageattn_hip_paged.h -- keeps
  //  its block table here: int32 [B, bt_stride], row b names the pages of batch b.  k, v and k_scale are then POOLS of pages:
  //  ksb / vsb / ks_b are the strides of a page, N = max_pages * page_size the logical capacity)
  union { int64_t msh; int32_t* pv_skipped; const int32_t* block_table; };
  // (causal split-KV -- attn_i8_splitkv_causal_kernel, sage_attn_splitkv_causal.hip -- keeps its fold g >= 1 in the third mask
  //  stride: query row r is token r / g, and the diagonal counts tokens)
  union { int64_t msm; int q_fold; };
  // (paged split-KV: the table's row stride in entries, in the word of the fourth mask stride)
  union { int64_t msn; int bt_stride; };
  union { int mask_kind; int bs_row; int num_splits; };
  // KV tile layout (sage_kv_layout, include/sageattn_hip.h): byte distance between consecutive 64-key tiles of one
  // (b, h_kv) in k8 and in v (always set by attn_check; the dense defaults are 64 rows), and the strides of k_scale
  // (floats) per batch, kv head and 64-key tile.  Sequence-parallel exchange buffers are tile-major: tile j of every
  // (b, h) is a contiguous block and the tiles of all ranks form one sequence.
  int k_tile_bytes, v_tile_bytes;
  int64_t ks_b, ks_h;
  int ks_t;
  // non-default tile strides (read by the host only; paged split-KV: log2 of the 64-key tiles per page, 0 .. 2)
  union { int kv_tiled; int bt_shift; };
  int o_vec16;   // every output row starts on a 16-byte boundary (all strides multiples of 8 elements): 16-byte stores
};

// K/V slots of the LDS tile ring (see the kernel): 4 for the FP8-PV loop where every wave copies a full share of each tile
constexpr int attn_ring_slots(int D, int nwaves, bool pv_fp8) { return (pv_fp8 && nwaves * 64 <= 4 * D) ? 4 : 2; }
// dynamic LDS of a launch in bytes: ring slots x (K tile + V tile); a tile is 64 keys of int8 K and of fp8 or 16-bit V
constexpr size_t attn_lds_bytes(int D, int nwaves, bool pv_fp8) {
  return (size_t)attn_ring_slots(D, nwaves, pv_fp8) * (64 * D + (pv_fp8 ? 64 * D : 64 * D * 2));
}

// dynamic LDS above the 48 KiB default needs the function attribute; its status is part of the launch status
__host__ inline bool allow_lds(const void* kern, size_t bytes) {
  launch_begin();
  return bytes <= 48 * 1024 ||
         hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

// entries a list row holds beyond its tiles: the deepest read-ahead of the attention loop (the four-slot ring copies K four
// positions ahead and requests that entry one iteration earlier)
constexpr int kBlockListPad = 5;
// int32 entries per list row for N keys: the count, ceil(N/64) tiles, the pad; rounded up so that every row starts on 16 bytes
constexpr int64_t block_list_row(int N) { return ((1 + ((int64_t)N + 63) / 64 + kBlockListPad) + 3) & ~(int64_t)3; }

// v_max_f32 on values that are never signalling NaNs: fmaxf() makes hipcc canonicalise both operands first
// (v_max_f32 x, x, x), two extra instructions on a kernel bound by the vector issue port
__device__ __forceinline__ float max_raw(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
#else
  return a > b ? a : b;
#endif
}
__device__ __forceinline__ float swap_max(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return max_raw(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float swap_sum(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// 16 bytes per lane, buffer -> LDS without passing through VGPRs (buffer_load_dwordx4 ... offen lds).
// Issued through inline asm ON PURPOSE: hipcc would otherwise treat the copy as a store that may alias every later
// LDS read and drain it with s_waitcnt vmcnt(0) a few instructions after issue.  Here nothing waits for it until
// dma_wait_all() in front of the workgroup barrier that publishes the tile, a whole iteration later.
// `lds_off` = byte offset of the wave's 1 KiB destination inside the workgroup's LDS (wave-uniform; lane l lands at
// +16*l), `rsrc` = buffer descriptor (4 uniform dwords), `voffset` per lane, `soffset` uniform.
__device__ __forceinline__ void lds_dma16(v4i rsrc, unsigned lds_off, int voffset, int soffset) {
#if defined(__HIP_DEVICE_COMPILE__)
  // M0 (the LDS base of the copy) is declared clobbered instead of saved and restored around the instruction: two scalar
  // moves less per copy (+0.2 ... +2 %, most on the short head_dim-64 tiles)
  asm volatile(
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %0, %1, %3 offen lds"
      :
      : "v"(voffset), "s"(rsrc), "s"(lds_off), "s"(soffset)
      : "memory", "m0");
#endif
}
// The same copy for a descriptor (or soffset) that was computed just in front of it -- the per-tile descriptors of the paged
// split-KV kernels.  Nothing inside an asm string is padded by the compiler: a buffer instruction that reads an SGPR written by
// a v_readfirstlane needs 5 wait states behind the write, and whether hipcc forms a descriptor word on the scalar ALU (no
// hazard) or moves it over from a VGPR is its choice per instantiation.  `s_nop 4` behind the M0 move gives 5 states (the move
// is a sixth), which covers that case and the one state M0 itself needs, whatever produced the operands.
__device__ __forceinline__ void lds_dma16_fresh(v4i rsrc, unsigned lds_off, int voffset, int soffset) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile(
      "s_mov_b32 m0, %2\n\t"
      "s_nop 4\n\t"
      "buffer_load_dwordx4 %0, %1, %3 offen lds"
      :
      : "v"(voffset), "s"(rsrc), "s"(lds_off), "s"(soffset)
      : "memory", "m0");
#endif
}
// counted form: wait until at most N of the wave's vector-memory operations are outstanding (they complete in order)
template <int N>
__device__ __forceinline__ void dma_wait_keep() {
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#endif
}
__device__ __forceinline__ void dma_wait_all() {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
}
// raw buffer descriptor as 4 provably wave-uniform dwords (gfx950: word3 = 0x00020000)
__device__ __forceinline__ v4i make_rsrc(const void* base, unsigned num_bytes) {
  const uint64_t a = reinterpret_cast<uint64_t>(base);
  v4i r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffu));
  r[1] = __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffu));
  r[2] = __builtin_amdgcn_readfirstlane((int)num_bytes);
  r[3] = 0x00020000;
  return r;
}

// Loads through the scalar cache (s_load, lgkmcnt) for wave-uniform addresses of read-only data: the constant
// address space cast is what lets hipcc pick SMEM; hidden from the host pass.
__device__ __forceinline__ float4 uniform_load4(const float* ptr) {
#if defined(__HIP_DEVICE_COMPILE__)
  const v4f v = *(const __attribute__((address_space(4))) v4f*)(ptr);
  return make_float4(v[0], v[1], v[2], v[3]);
#else
  return make_float4(0.f, 0.f, 0.f, 0.f);
#endif
}
__device__ __forceinline__ int uniform_load_i32(const int* ptr) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const __attribute__((address_space(4))) int*)(ptr);
#else
  return 0;
#endif
}
__device__ __forceinline__ float uniform_load1(const float* ptr) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const __attribute__((address_space(4))) float*)(ptr);
#else
  return 0.f;
#endif
}

// raw buffer descriptor from values that ARE wave-uniform by construction (kernel arguments, workgroup ids, scalar loads):
// no readfirstlane, the words stay on the scalar unit
__device__ __forceinline__ v4i make_rsrc_uniform(const uint64_t a, const unsigned num_bytes) {
  v4i r;
  r[0] = (int)(a & 0xffffffffu);
  r[1] = (int)((a >> 32) & 0xffffu);
  r[2] = (int)num_bytes;
  r[3] = 0x00020000;
  return r;
}

template <int D>
__device__ __forceinline__ int k_swz(int row) {
  // 16-B chunk XOR that makes the ds_read_b128 A-fragment reads conflict free
  if constexpr (D == 128) return (row >> 1) & 7; else return (row >> 2) & 3;
}
template <int D>
__device__ __forceinline__ int v_win_swz(int row) {
  // 64-B window XOR for the fp16 V tile so that the 4 rows of a tr-read land on 4 windows
  if constexpr (D == 128) return row & 3; else return (row >> 1) & 1;
}

}  // namespace sage
