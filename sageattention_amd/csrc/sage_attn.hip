// Fused INT8-QK^T -> online softmax -> FP16/FP8-PV attention for gfx950 (MI355X, CDNA4).
//
// Replaces the tile loop of csrc/qattn/qk_int_sv_f16_cuda_sm80.cu:44-671 and
// csrc/qattn/qk_int_sv_f8_cuda_sm89.cuh:44-713 (semantics), designed for wave64 + MFMA:
//
//  * one wave owns 32 query rows; a workgroup of NWAVES waves owns NWAVES*32 rows and shares the
//    K/V tiles (64 keys) through an LDS ring (two slots, four for FP8 PV) filled by LDS-DMA (buffer_load ... lds): a
//    copy is issued one to four tiles ahead and drained by a counted s_waitcnt in front of the barrier that publishes it,
//    so HBM/L2 latency hides under the MFMA phases and no VGPR is spent on staging.
//  * S^T = K . Q^T on v_mfma_i32_32x32x32_i8 (A = K tile rows from LDS via ds_read_b128, B = Q^T held in
//    registers for the whole kernel).  With this orientation every lane owns ONE query row
//    (column of S^T): 32 of the 64 scores of its row sit in its own registers, the other 32 in
//    lane^32, so the row max needs one v_permlane32_swap and the row sum none until the end.
//  * P^T stays in registers: the fp32 accumulator layout of S^T is, after a packed fp16 convert,
//    exactly the B operand of O^T += V^T . P^T on v_mfma_f32_32x32x16_f16; V^T fragments come
//    from the row-major V tile in LDS through ds_read_b64_tr_b16 (hardware transpose).
//  * O^T (d in registers, query row on the lane) is rescaled per lane, normalised and stored.
//
// Roofline: MFMA (4*M*N*D flop per (b,h); half int8 at 2x the fp16 rate), VALU/exp2 co-limited.
// Algorithmic HBM bytes per (b,h): M*D (Q) + N*D (K) + 2*N*D (V fp16) + 2*M*D (O) + scales.
#include "sage_attn_launch.h"

namespace sage {

// PV_FP8 = false: V fp16 [N][D] row major, PV on v_mfma_f32_32x32x16_f16.  V_BF16: V stays bf16 -- P is packed to bf16
//                 (v_cvt_pk_bf16_f32) and P.V runs on v_mfma_f32_32x32x16_bf16, so the tile is staged and read exactly
//                 like an fp16 one and nothing is converted (the reference converts V to fp16 first, core.py:633).
// PV_FP8 = true : V^T OCP e4m3 [D][Npad] in MFMA token order (sage_fp8.hip), PV on the MX-scaled
//                 v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales (2x the fp16 rate), P in e4m3.
//
// SPARSE = true: the block-sparse form (attn_i8_blocksparse_kernel below).  The workgroup's 128 query rows are one block row
//                 of the caller's block map, and the tile loop walks that row's ascending list of active 64-key tiles
//                 (sage_block_map_compact) instead of 0 .. ntiles-1: list POSITION t drives ring slots, unroll parity and
//                 the plain / tail split exactly as the tile index does in the dense kernel, list ENTRY t is the tile that is
//                 copied, whose scales are loaded and whose sequence end is masked.  Entries are wave uniform: they come
//                 through the scalar cache and live in SGPRs.
// The loop body lives in sage_attn_body.h and is included into both kernels, so attn_i8_kernel keeps its template
// parameter list (the build's occupancy guard and tests/test_build_guards.py match its mangled name) AND its code: shared
// through a __device__ __forceinline__ template instead, every dense instantiation came out with another register
// allocation (head_dim 64 bf16 V: 166 -> 178 VGPRs, over the three-waves-per-SIMD line).
template <int D, int NWAVES, bool CAUSAL, bool KTHREAD, bool V_BF16, bool PV_FP8, bool HAS_MASK>
// (head_dim 64 FP8 PV in its dispatched 4-wave geometry is told to stay within 168 registers = three waves per SIMD: it fits
//  without scratch, but left alone hipcc settles a few registers above the line)
__global__ __launch_bounds__(NWAVES * 64, (D == 64 && PV_FP8 && NWAVES == 4) ? 3 : 2)
void attn_i8_kernel(const AttnParams p) {
  constexpr bool SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = false, PAGED = false;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// Block-sparse attention: the same loop body over the active tiles of a block map (see SPARSE above).  Always four waves:
// a workgroup's 128 rows are exactly one block row of the map.
template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_blocksparse_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = false, HAS_MASK = false, SPARSE = true, PVSKIP = false, KVLEN = false, SPLITKV = false, PAGED = false;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// (attn_i8_blocksparse_pvskip_kernel, the twin with SpargeAttn's second stage -- PVSKIP = true -- is built from the same body
//  in sage_attn_pvskip.hip: a file of its own because it needs a compiler option of its own, see there)
// (attn_i8_kvlen_kernel, the dense kernel with per-batch key lengths -- KVLEN = true -- is built from the same body in
//  sage_attn_kvlen.hip: as many instantiations again as attn_i8_kernel has without attn_mask, compiled beside this file)
// (attn_i8_blocksparse_kvlen_kernel and attn_i8_blocksparse_pvskip_kvlen_kernel, the block-sparse kernels with per-batch key
//  lengths -- SPARSE and KVLEN -- are built from the same body in sage_attn_sparse_kvlen.hip and sage_attn_sparse_kvlen_pvskip.hip)

// The rows of the empty q-blocks of a block-sparse call (no active tile: the attention kernel returns at once): o = 0,
// lse = -inf, and with skip counters (pv_skipped, else null) the four counters of the q-block = 0.  One workgroup per list
// row; all but the empty ones leave after one scalar load.
__global__ __launch_bounds__(256) void attn_blocksparse_empty_kernel(const AttnParams p, const int D) {
  const int qb = blockIdx.x % p.nqb, bh = blockIdx.x / p.nqb;
  if (uniform_load_i32(p.bs_lists + (int64_t)blockIdx.x * p.bs_row) > 0) return;
  const int h = bh % p.Hq, b = bh / p.Hq;
  const int rows = min(128, p.M - qb * 128), per_row = D / 4;
  uint16_t* ob = p.o + b * p.osb + h * p.osh + (int64_t)(qb * 128) * p.osn;
  for (int i = threadIdx.x; i < rows * per_row; i += 256)
    *reinterpret_cast<uint2*>(ob + (int64_t)(i / per_row) * p.osn + (i % per_row) * 4) = make_uint2(0u, 0u);
  if (p.lse && (int)threadIdx.x < rows) p.lse[((int64_t)b * p.Hq + h) * p.M + qb * 128 + threadIdx.x] = -INFINITY;
  if (p.pv_skipped && threadIdx.x < 4) p.pv_skipped[(int64_t)blockIdx.x * 4 + threadIdx.x] = 0;
}

template <int D, int NWAVES, bool CAUSAL, bool KTHREAD, bool V_BF16, bool PV_FP8, bool HAS_MASK>
static int launch_kernel(const AttnParams& p, size_t smem, hipStream_t st) {
  auto kern = attn_i8_kernel<D, NWAVES, CAUSAL, KTHREAD, V_BF16, PV_FP8, HAS_MASK>;
  if (!allow_lds((const void*)kern, smem)) return SAGE_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, dim3(p.nqb * p.Hq * p.B), dim3(NWAVES * 64), smem, st, p);
  return launch_status();
}

// block-sparse form: the kernel, or its twin with the P.V skip (sage_attn_pvskip.hip), then the rows of the empty q-blocks
static int launch_blocksparse(const AttnCall& c, hipStream_t st) {
  if (c.sparse_kvlen) return launch_blocksparse_kvlen(c, st);  // ... with key lengths: kernels and empty rows of their own
  const int grid = c.p.nqb * c.p.Hq * c.p.B;
  const int s = c.pvskip ? launch_blocksparse_pvskip(c, st) : launch_4wave_kernel(c, st, grid, [](auto d, auto k, auto v, auto fp8) {
    return attn_i8_blocksparse_kernel<decltype(d)::value, decltype(k)::value, decltype(v)::value, decltype(fp8)::value>;
  });
  if (s) return s;
  hipLaunchKernelGGL(attn_blocksparse_empty_kernel, dim3(grid), dim3(256), 0, st, c.p, c.D);
  return launch_status();
}

template <int D, int NWAVES>
static int launch_attn(const AttnCall& c, hipStream_t st) {
  const AttnParams& p = c.p;
  return by_flag(c.pv_fp8, [&](auto fp8) {
    constexpr bool PV_FP8 = decltype(fp8)::value;
    // V element type: fp8 V has no bf16 flavour
    auto by_v = [&](auto f) { if constexpr (PV_FP8) return f(std::false_type{}); else return by_flag(c.v_bf16, f); };
    if constexpr (!PV_FP8) {
      if (p.mask) {  // attn_mask variant (non-causal, fp16 V: checked by attn_check)
        const size_t smem = attn_lds_bytes(D, NWAVES, false);
        return by_flag(c.kthread, [&](auto k) {
          return by_v([&](auto v) {
            return launch_kernel<D, NWAVES, false, decltype(k)::value, decltype(v)::value, false, true>(p, smem, st);
          });
        });
      }
    }
    const size_t smem = attn_lds_bytes(D, NWAVES, PV_FP8);
    return by_flag(c.causal, [&](auto ca) {
      return by_flag(c.kthread, [&](auto k) {
        return by_v([&](auto v) {
          return launch_kernel<D, NWAVES, decltype(ca)::value, decltype(k)::value, decltype(v)::value, PV_FP8, false>(p, smem, st);
        });
      });
    });
  });
}

// tuning hook (sage_set_tuning): per host thread, so a test or tool that pins the geometry for its own calls cannot change
// the launches of another thread; 0 = the measured default below
static thread_local int g_nwaves_override = 0;

// argument checks of the attention entry points; fills the kernel parameters and the geometry
int attn_check(AttnCall& c, const AttnArgs& a) {
  const float* q_scale = a.q_scale;
  int warpq = a.warpq;
  const bool sparse = a.block_sparse;
  if (sparse) {  // a block map combines with none of the other forms; its lists are read 16 bytes aligned rows
    if (!a.block_lists || !aligned16(a.block_lists)) return SAGE_ERR_INVALID_ARGUMENT;
    if (a.pv_skip && (!a.pv_thresh || ((uintptr_t)a.pv_thresh & 3) || ((uintptr_t)a.pv_skipped & 3)))
      return SAGE_ERR_INVALID_ARGUMENT;
    if (a.block_key_lens && (!a.block_kv_lens || ((uintptr_t)a.block_kv_lens & 3))) return SAGE_ERR_INVALID_ARGUMENT;
    if (a.is_causal || a.cu_q || a.cu_k || a.mask || a.kvl || a.v_mean) return SAGE_ERR_UNSUPPORTED;
  } else if (a.block_key_lens) {
    return SAGE_ERR_UNSUPPORTED;  // the lengths of the block-sparse form without its lists
  }
  if (a.key_lens) {  // per-batch key lengths: the dense padded layout only; read on the device as aligned int32
    if (!a.kv_lens || ((uintptr_t)a.kv_lens & 3)) return SAGE_ERR_INVALID_ARGUMENT;
    if (sparse || a.mask || a.cu_q || a.cu_k || a.kvl) return SAGE_ERR_UNSUPPORTED;
  }
  if (a.split_kv) {  // split-KV: the fused-Q dense padded form only; its workspace is read and written 16 bytes aligned
    if (a.num_splits < 1 || a.num_splits > SAGE_MERGE_MAX || !a.split_workspace || !aligned16(a.split_workspace) ||
        ((uintptr_t)a.split_kv_lens & 3) || (a.split_causal && (a.q_fold < 1 || a.M % a.q_fold != 0)))
      return SAGE_ERR_INVALID_ARGUMENT;
    if (sparse || a.key_lens || a.is_causal || a.mask || a.cu_q || a.cu_k || a.kvl || a.v_mean || a.q_dtype < 0 || !a.km)
      return SAGE_ERR_UNSUPPORTED;
  }
  if (a.paged && !a.split_kv) return SAGE_ERR_UNSUPPORTED;  // block tables: the split-KV form only
  if (a.mask && (a.mask_kind < 1 || a.mask_kind > 3 || !a.mask_strides || a.is_causal || a.pv_fp8 || a.cu_q)) return SAGE_ERR_INVALID_ARGUMENT;
  const bool fusedq = a.q_dtype >= 0;  // a.q is then the fp16/bf16 query tensor
  if ((a.cu_q == nullptr) != (a.cu_k == nullptr)) return SAGE_ERR_INVALID_ARGUMENT;
  if (fusedq) {
    if (a.q_dtype != SAGE_F16 && a.q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
    if (a.qk_gran == SAGE_GRAN_PER_BLOCK || a.cu_q || (a.km && !aligned16(a.km))) return SAGE_ERR_UNSUPPORTED;
    if (!tensor_ok(a.q, 8) || !a.k_scale) return SAGE_ERR_INVALID_ARGUMENT;
    q_scale = a.k_scale;  // unused placeholder so the shared checks below pass
  }
  if (a.cu_q && (a.pv_fp8 || a.lse)) return SAGE_ERR_UNSUPPORTED;  // packed sequences: fp16 PV, no LSE (as the reference)
  if (!tensor_ok(a.q, fusedq ? 8 : 16) || !tensor_ok(a.k8, 16) || !tensor_ok(a.v, a.pv_fp8 ? 16 : 8) || !tensor_ok(a.o, 4) || !q_scale ||
      !a.k_scale)
    return SAGE_ERR_INVALID_ARGUMENT;
  if (a.pv_fp8 && !a.v_scale) return SAGE_ERR_INVALID_ARGUMENT;
  if (a.B <= 0 || a.Hq <= 0 || a.Hk <= 0 || a.M <= 0 || a.N <= 0 || a.Hq % a.Hk != 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (sparse && a.block_lists_bytes < block_sparse_bytes(a.B, a.Hq, a.M, a.N)) return SAGE_ERR_INVALID_ARGUMENT;
  // the integer row max and the -inf mask pattern rely on a positive, finite dequantisation scale
  if (!a.logit_mult_is_one && !(a.sm_scale > 0.f && a.sm_scale < 1.0e30f)) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = dim_dtype_status(a.D, a.v_dtype)) return s;
  if (a.split_kv && (int64_t)a.split_workspace_bytes < splitkv_bytes(a.B, a.Hq, a.M, a.D, a.num_splits)) return SAGE_ERR_INVALID_ARGUMENT;
  if (a.o_dtype != SAGE_F16 && a.o_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  if (a.qk_gran < SAGE_GRAN_PER_BLOCK || a.qk_gran > SAGE_GRAN_PER_THREAD) return SAGE_ERR_INVALID_ARGUMENT;
  if (a.blkq != 64 && a.blkq != 128) return SAGE_ERR_INVALID_ARGUMENT;
  if (a.qk_gran == SAGE_GRAN_PER_BLOCK) warpq = a.blkq;
  if ((warpq != 16 && warpq != 32 && warpq != 64 && warpq != 128) || a.blkq % warpq != 0) return SAGE_ERR_INVALID_ARGUMENT;
  if ((a.v_mean && !aligned16(a.v_mean)) || (a.v_scale && !aligned16(a.v_scale))) return SAGE_ERR_INVALID_ARGUMENT;
  // KV tile layout: dense by default (a tile = 64 consecutive rows of the sage_tensor), explicit for tile-major buffers
  // (paged: the tiles of one PAGE -- a (page, head) slice is what the strides of the scales and the window below describe)
  const int64_t ntile = a.paged ? a.page_size / 64 : ((int64_t)a.N + 63) >> 6;
  int64_t k_tile = 64 * a.k8->stride_n, v_tile = a.pv_fp8 ? 64 : 128 * a.v->stride_n;  // bytes
  const int per_tile = a.qk_gran == SAGE_GRAN_PER_THREAD ? 4 : 1;
  int64_t ks_h = ntile * per_tile, ks_b = ks_h * a.Hk, ks_t = per_tile;
  bool tiled = false;
  if (a.kvl) {
    if (a.cu_q || a.mask || a.kvl->k_tile_stride < 0 || a.kvl->v_tile_stride < 0) return SAGE_ERR_INVALID_ARGUMENT;
    if (a.kvl->k_tile_stride) { k_tile = a.kvl->k_tile_stride; tiled = true; }
    if (a.kvl->v_tile_stride) { v_tile = a.pv_fp8 ? a.kvl->v_tile_stride : 2 * a.kvl->v_tile_stride; tiled = true; }
    if (a.kvl->ks_stride_b || a.kvl->ks_stride_h || a.kvl->ks_stride_tile) {
      if (a.kvl->ks_stride_tile < per_tile || a.kvl->ks_stride_h < 0 || a.kvl->ks_stride_b < 0) return SAGE_ERR_INVALID_ARGUMENT;
      ks_b = a.kvl->ks_stride_b; ks_h = a.kvl->ks_stride_h; ks_t = a.kvl->ks_stride_tile;
      if (per_tile == 4 && ((ks_b | ks_h | ks_t) & 3)) return SAGE_ERR_INVALID_ARGUMENT;  // 16-B scalar loads
    }
    if ((k_tile & 15) || (v_tile & 15)) return SAGE_ERR_INVALID_ARGUMENT;
  }
  // the K/V slices of one (b, h_kv) are addressed with 32-bit buffer offsets
  const int64_t lim = (int64_t)1 << 31;
  if (ntile * k_tile + 64 * a.k8->stride_n + a.D >= lim) return SAGE_ERR_TOO_LARGE;
  if (a.pv_fp8 ? (ntile * v_tile + (int64_t)a.D * a.v->stride_n + 64 >= lim) : (ntile * v_tile + (64 * a.v->stride_n + a.D) * 2 >= lim)) return SAGE_ERR_TOO_LARGE;
  if (ks_t * ntile >= lim) return SAGE_ERR_TOO_LARGE;
  AttnParams& p = c.p;
  p.q = (const int8_t*)a.q->data; p.qsb = a.q->stride_b; p.qsh = a.q->stride_h; p.qsn = a.q->stride_n;
  p.k = (const int8_t*)a.k8->data; p.ksb = a.k8->stride_b; p.ksh = a.k8->stride_h; p.ksn = a.k8->stride_n;
  p.v = (const uint8_t*)a.v->data; p.vsb = a.v->stride_b; p.vsh = a.v->stride_h; p.vsn = a.v->stride_n;
  p.o = (uint16_t*)a.o->data; p.osb = a.o->stride_b; p.osh = a.o->stride_h; p.osn = a.o->stride_n;
  p.q_scale = q_scale; p.k_scale = a.k_scale; p.v_scale = a.v_scale; p.v_mean = a.v_mean; p.lse = a.lse;
  p.B = a.B; p.Hq = a.Hq; p.Hk = a.Hk; p.M = a.M; p.N = a.N;
  const int nblkq = (a.M + a.blkq - 1) / a.blkq;
  p.gq = a.qk_gran == SAGE_GRAN_PER_BLOCK ? nblkq : a.qk_gran == SAGE_GRAN_PER_WARP ? nblkq * (a.blkq / warpq) : nblkq * (a.blkq / warpq) * 8;
  const int nblkk = (a.N + 63) / 64;
  p.gk = a.qk_gran == SAGE_GRAN_PER_THREAD ? nblkk * 4 : nblkk;
  p.qgran = a.qk_gran; p.blkq = a.blkq; p.warpq = warpq;
  p.logit_mult = a.logit_mult_is_one ? 1.0f : a.sm_scale * kLog2e;
  p.out_bf16 = a.o_dtype == SAGE_BF16;
  p.cu_q = a.cu_q; p.cu_k = a.cu_k;
  p.mask = (const uint8_t*)a.mask; p.mask_kind = a.mask ? a.mask_kind : 0;
  const int64_t* const ms = a.mask_strides;
  p.msb = a.mask ? ms[0] : 0; p.msh = a.mask ? ms[1] : 0; p.msm = a.mask ? ms[2] : 0; p.msn = a.mask ? ms[3] : 0;
  p.k_tile_bytes = (int)k_tile; p.v_tile_bytes = (int)v_tile; p.ks_b = ks_b; p.ks_h = ks_h; p.ks_t = (int)ks_t;
  p.kv_tiled = tiled ? 1 : 0;
  p.o_vec16 = (a.o->stride_b % 8 == 0 && a.o->stride_h % 8 == 0 && a.o->stride_n % 8 == 0) ? 1 : 0;  // 16-byte aligned output rows
  p.q_f16 = fusedq ? (const uint16_t*)a.q->data : nullptr;
  p.km = (const uint16_t*)a.km; p.q_bf16 = a.q_dtype == SAGE_BF16; p.sm_scale = a.sm_scale;
  // measured on MI355X: D=128 fp16 PV -> one 8-wave workgroup per CU (4-wave: -3 %); D=128 fp8 PV -> two 4-wave
  // workgroups per CU (+3.6 % non-causal, +5.7 % causal); D=64 (<= 168 VGPRs) -> 4-wave workgroups, 3 per CU
  // ... except for short key sequences (few tiles per workgroup, so prologue and epilogue weigh more and two smaller
  // workgroups per CU overlap them better): end to end, 4-wave 0.959x the 8-wave time at 2048 keys, 0.979x at 3072, 0.998x
  // at 4096, 1.02x from 6144; causal 0.993x at 8192 (4096 keys per row on average) -> 4 waves up to 3072 keys per row
  // (profiles/r03_ab/geometry_end_to_end.log).
  const int keys_per_row = a.is_causal ? a.N / 2 : a.N;
  // FP8 PV at head_dim 128: 4-wave workgroups +2.2 % at 8K keys, +0.7 % at 16K, -1.1 % at 32K, -1.3 % at 64K.  The two
  // co-resident 4-wave workgroups of a CU drift apart on a long stream until they no longer share K/V tiles in L2 (1.90x the
  // algorithmic HBM-side bytes with 4 waves, 1.00x with 8: profiles/r03_ab/fetch_by_geometry.md) -> 8 waves beyond 24K keys per row.
  // (block-sparse: always 4 waves -- a workgroup is one block row of the map; the tuning knobs do not apply)
  // (split-KV: always 4 waves as well -- its workgroups are there to fill the chip, and the partials are defined by the 4-wave loop)
  const int nw = (sparse || a.split_kv) ? 4
                 : a.nwaves            ? a.nwaves
                 : g_nwaves_override ? g_nwaves_override
                                     : ((a.D == 64 || (a.pv_fp8 && keys_per_row <= 24576) || keys_per_row <= 3072) ? 4 : 8);
  p.nqb = (a.M + nw * 32 - 1) / (nw * 32);
  if (sparse) { p.bs_lists = a.block_lists; p.bs_row = (int)block_list_row(a.N); }  // (share the words of mask / mask_kind)
  c.pvskip = sparse && a.pv_skip;
  if (c.pvskip) { p.pv_thresh = a.pv_thresh; p.pv_skipped = a.pv_skipped; }  // (... and those of two mask strides)
  c.kvlen = a.key_lens;
  if (c.kvlen) p.kv_lens = a.kv_lens;  // (shares the word of cu_k, null here)
  c.sparse_kvlen = sparse && a.block_key_lens;
  if (c.sparse_kvlen) p.kv_lens = a.block_kv_lens;  // (the word of cu_k again: the block-sparse form has no packed sequences)
  c.splitkv = a.split_kv;
  if (c.splitkv) {  // (the words of mask, its first stride, mask_kind and cu_k, all unused here)
    p.sk_o = (float*)a.split_workspace;
    p.sk_lse = p.sk_o + (int64_t)a.num_splits * a.B * a.Hq * a.M * a.D;
    p.num_splits = a.num_splits;
    p.kv_lens = a.split_kv_lens;
    if (a.split_causal) p.q_fold = a.q_fold;  // (... and the word of the third mask stride)
  }
  c.splitkv_causal = a.split_kv && a.split_causal;
  c.paged = a.paged;
  if (c.paged) {  // (the words of the second and fourth mask stride and of kv_tiled, which only the host reads)
    p.block_table = a.block_table;
    p.bt_stride = a.table_stride;
    p.bt_shift = a.page_size == 64 ? 0 : a.page_size == 128 ? 1 : 2;
  }
  c.D = a.D; c.nwaves = nw; c.sparse = sparse;
  c.pv_fp8 = a.pv_fp8; c.causal = a.is_causal != 0; c.kthread = a.qk_gran == SAGE_GRAN_PER_THREAD; c.v_bf16 = a.v_dtype == SAGE_BF16;
  return SAGE_OK;
}

int attn_launch(const AttnCall& c, hipStream_t st) {
  if (c.sparse) return launch_blocksparse(c, st);
  if (c.kvlen) return launch_kvlen(c, st);
  if (c.splitkv) {  // the attention kernel over (b, h, q-block, split), causal or not, then the merge
    const int s = c.paged ? (c.splitkv_causal ? launch_splitkv_causal_paged_attn(c, st) : launch_splitkv_paged_attn(c, st))
                          : (c.splitkv_causal ? launch_splitkv_causal_attn(c, st) : launch_splitkv_attn(c, st));
    return s ? s : launch_splitkv_merge(c, st);
  }
  return by_dim(c.D, [&](auto d) {
    return c.nwaves == 8 ? launch_attn<decltype(d)::value, 8>(c, st) : launch_attn<decltype(d)::value, 4>(c, st);
  });
}

// the public entry points: check, then launch
static int run_attn(const AttnArgs& a, sage_stream_t stream) {
  AttnCall c;
  if (const int s = attn_check(c, a)) return s;
  return attn_launch(c, (hipStream_t)stream);
}

// The argument block of an entry point, filled from what the forms of its family share: {INT8 Q, fused Q} x {FP16 / BF16 V,
// FP8 V}.  Parameters in the order of the C signatures.  The one fill is that of INT8 Q with FP16 / BF16 V; the other three
// families go through it and add what is theirs.
static AttnArgs int8_f16_args(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, int v_dtype, const sage_tensor* o,
                              int o_dtype, const float* q_scale, const float* k_scale, const float* v_mean, float* lse, int B,
                              int Hq, int Hk, int M, int N, int D, int is_causal, int qk_gran, int blkq, int warpq,
                              float sm_scale, int logit_mult_is_one) {
  AttnArgs a;
  a.q = q8; a.k8 = k8; a.v = v; a.v_dtype = v_dtype; a.o = o; a.o_dtype = o_dtype; a.q_scale = q_scale; a.k_scale = k_scale;
  a.v_mean = v_mean; a.lse = lse; a.B = B; a.Hq = Hq; a.Hk = Hk; a.M = M; a.N = N; a.D = D; a.is_causal = is_causal;
  a.qk_gran = qk_gran; a.blkq = blkq; a.warpq = warpq; a.sm_scale = sm_scale; a.logit_mult_is_one = logit_mult_is_one;
  return a;
}

// FP8 V: v is the FP8 V^T (v_dtype keeps its default), v_scale its scales
static AttnArgs int8_f8_args(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8, const sage_tensor* o,
                             int o_dtype, const float* q_scale, const float* k_scale, const float* v_scale, const float* v_mean,
                             float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal, int qk_gran, int blkq,
                             int warpq, float sm_scale, int logit_mult_is_one) {
  AttnArgs a = int8_f16_args(q8, k8, v_fp8, SAGE_F16, o, o_dtype, q_scale, k_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                             qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  a.pv_fp8 = true; a.v_scale = v_scale;
  return a;
}

// the fused-Q forms: q is the fp16 / bf16 query tensor (no q_scale), km the k_mean of the LSE correction; 128-row q-blocks,
// and the kernel applies sm_scale.  `status` is that of q_dtype: an entry point returns it, if not SAGE_OK, before it goes on
static AttnArgs fusedq_f16_args(int& status, const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v,
                                int v_dtype, const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal,
                                int qk_gran, int warpq, float sm_scale) {
  AttnArgs a = int8_f16_args(q, k8, v, v_dtype, o, o_dtype, nullptr, k_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal, qk_gran,
                             128, warpq, sm_scale, 0);
  a.q_dtype = q_dtype; a.km = km;
  status = q_dtype != SAGE_F16 && q_dtype != SAGE_BF16 ? SAGE_ERR_INVALID_ARGUMENT : SAGE_OK;
  return a;
}

static AttnArgs fusedq_f8_args(int& status, const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_fp8,
                               const sage_tensor* o, int o_dtype, const float* k_scale, const void* km, const float* v_scale,
                               const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal,
                               int qk_gran, int warpq, float sm_scale) {
  AttnArgs a = fusedq_f16_args(status, q, q_dtype, k8, v_fp8, SAGE_F16, o, o_dtype, k_scale, km, v_mean, lse, B, Hq, Hk, M, N, D,
                               is_causal, qk_gran, warpq, sm_scale);
  a.pv_fp8 = true; a.v_scale = v_scale;
  return a;
}

// the block-sparse forms: the tile lists of sage_block_map_compact
static void block_sparse(AttnArgs& a, const int32_t* block_lists, int64_t block_lists_bytes) {
  a.block_sparse = true; a.block_lists = block_lists; a.block_lists_bytes = block_lists_bytes;
}

// ... with the P.V skip: the per-head thresholds and the skip counters
static void pv_skip(AttnArgs& a, const float* pv_thresh, int32_t* skipped) {
  a.pv_skip = true; a.pv_thresh = pv_thresh; a.pv_skipped = skipped;
}

// the forms with per-batch key lengths: batch b attends its keys [0, clamp(kv_lens[b], 0, N))
static void key_lens(AttnArgs& a, const int32_t* kv_lens) {
  a.key_lens = true; a.kv_lens = kv_lens;
}

// the block-sparse forms with per-batch key lengths: the lists, the P.V skip iff pv_thresh is given, the lengths
static void block_sparse_key_lens(AttnArgs& a, const int32_t* block_lists, int64_t block_lists_bytes, const float* pv_thresh,
                                  int32_t* skipped, const int32_t* kv_lens) {
  block_sparse(a, block_lists, block_lists_bytes);
  if (pv_thresh) pv_skip(a, pv_thresh, skipped);
  a.block_key_lens = true; a.block_kv_lens = kv_lens;
}

}  // namespace sage

using namespace sage;

extern "C" int sage_set_tuning(int key, int value) {
  if (key == SAGE_TUNE_NWAVES) {
    if (value != 0 && value != 4 && value != 8) return SAGE_ERR_INVALID_ARGUMENT;
    g_nwaves_override = value;
    return SAGE_OK;
  }
  return SAGE_ERR_INVALID_ARGUMENT;
}

extern "C" int sage_get_tuning(int key) {
  if (key == SAGE_TUNE_NWAVES) return g_nwaves_override;
  return -1;
}

extern "C" int sage_attn_qk_int8_pv_f16(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                        const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                        const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                        int is_causal, int qk_gran, int blkq, int warpq, float sm_scale,
                                        int logit_mult_is_one, sage_stream_t stream) {
  AttnArgs a = int8_f16_args(q8, k8, v, v_dtype, o, o_dtype, q_scale, k_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                             qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  return run_attn(a, stream);
}

extern "C" int sage_attn_qk_int8_pv_f8(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                       const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                       const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                       int N, int D, int is_causal, int qk_gran, int blkq, int warpq, float sm_scale,
                                       int logit_mult_is_one, sage_stream_t stream) {
  AttnArgs a = int8_f8_args(q8, k8, v_fp8, o, o_dtype, q_scale, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                            qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  return run_attn(a, stream);
}

extern "C" int sage_attn_qk_int8_pv_f16_varlen(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                               const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                               const int* cu_seqlens_q, const int* cu_seqlens_k, int num_seqs, int Hq, int Hk,
                                               int max_seqlen_q, int max_seqlen_k, int D, int is_causal, int qk_gran, int blkq,
                                               int warpq, float sm_scale, int logit_mult_is_one, sage_stream_t stream) {
  if (!cu_seqlens_q || !cu_seqlens_k) return SAGE_ERR_INVALID_ARGUMENT;
  AttnArgs a = int8_f16_args(q8, k8, v, v_dtype, o, o_dtype, q_scale, k_scale, /*v_mean*/ nullptr, /*lse*/ nullptr, num_seqs, Hq,
                             Hk, max_seqlen_q, max_seqlen_k, D, is_causal, qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  a.cu_q = cu_seqlens_q; a.cu_k = cu_seqlens_k;
  return run_attn(a, stream);
}

extern "C" int sage_attn_fusedq_pv_f16(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                       const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                       const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                       int is_causal, int qk_gran, int warpq, float sm_scale, sage_stream_t stream) {
  int status;
  AttnArgs a = fusedq_f16_args(status, q, q_dtype, k8, v, v_dtype, o, o_dtype, k_scale, km, v_mean, lse, B, Hq, Hk, M, N, D,
                               is_causal, qk_gran, warpq, sm_scale);
  if (status) return status;
  return run_attn(a, stream);
}

extern "C" int sage_attn_fusedq_pv_f8(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_fp8,
                                      const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                      const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                      int N, int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                                      sage_stream_t stream) {
  int status;
  AttnArgs a = fusedq_f8_args(status, q, q_dtype, k8, v_fp8, o, o_dtype, k_scale, km, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                              is_causal, qk_gran, warpq, sm_scale);
  if (status) return status;
  return run_attn(a, stream);
}

extern "C" int sage_attn_qk_int8_pv_f16_masked(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                               const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                               const void* attn_mask, int mask_kind, const int64_t* mask_strides, float* lse,
                                               int B, int Hq, int Hk, int M, int N, int D, int qk_gran, int blkq, int warpq,
                                               float sm_scale, int logit_mult_is_one, sage_stream_t stream) {
  if (!attn_mask) return SAGE_ERR_INVALID_ARGUMENT;
  AttnArgs a = int8_f16_args(q8, k8, v, v_dtype, o, o_dtype, q_scale, k_scale, /*v_mean*/ nullptr, lse, B, Hq, Hk, M, N, D,
                             /*is_causal*/ 0, qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  a.mask = attn_mask; a.mask_kind = mask_kind; a.mask_strides = mask_strides;
  return run_attn(a, stream);
}

extern "C" int sage_attn_qk_int8_pv_f16_kvtiles(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                                const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                                const sage_kv_layout* kv_layout, float* lse, int B, int Hq, int Hk, int M,
                                                int N, int D, int is_causal, int qk_gran, int blkq, int warpq, float sm_scale,
                                                sage_stream_t stream) {
  if (!kv_layout) return SAGE_ERR_INVALID_ARGUMENT;
  AttnArgs a = int8_f16_args(q8, k8, v, v_dtype, o, o_dtype, q_scale, k_scale, /*v_mean*/ nullptr, lse, B, Hq, Hk, M, N, D,
                             is_causal, qk_gran, blkq, warpq, sm_scale, /*logit_mult_is_one*/ 0);
  a.kvl = kv_layout;
  return run_attn(a, stream);
}

extern "C" int sage_attn_qk_int8_pv_f8_kvtiles(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                               const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                               const float* v_scale, const sage_kv_layout* kv_layout, float* lse, int B,
                                               int Hq, int Hk, int M, int N, int D, int is_causal, int qk_gran, int blkq,
                                               int warpq, float sm_scale, sage_stream_t stream) {
  if (!kv_layout) return SAGE_ERR_INVALID_ARGUMENT;
  AttnArgs a = int8_f8_args(q8, k8, v_fp8, o, o_dtype, q_scale, k_scale, v_scale, /*v_mean*/ nullptr, lse, B, Hq, Hk, M, N, D,
                            is_causal, qk_gran, blkq, warpq, sm_scale, /*logit_mult_is_one*/ 0);
  a.kvl = kv_layout;
  return run_attn(a, stream);
}

// ---- block-sparse forms: the dense twins' arguments plus the tile lists of sage_block_map_compact
extern "C" int sage_attn_qk_int8_pv_f16_blocksparse(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v,
                                                    int v_dtype, const sage_tensor* o, int o_dtype, const float* q_scale,
                                                    const float* k_scale, const float* v_mean, float* lse, int B, int Hq,
                                                    int Hk, int M, int N, int D, int is_causal, int qk_gran, int blkq,
                                                    int warpq, float sm_scale, int logit_mult_is_one,
                                                    const int32_t* block_lists, int64_t block_lists_bytes,
                                                    sage_stream_t stream) {
  AttnArgs a = int8_f16_args(q8, k8, v, v_dtype, o, o_dtype, q_scale, k_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                             qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  block_sparse(a, block_lists, block_lists_bytes);
  return run_attn(a, stream);
}

extern "C" int sage_attn_qk_int8_pv_f8_blocksparse(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                                   const sage_tensor* o, int o_dtype, const float* q_scale,
                                                   const float* k_scale, const float* v_scale, const float* v_mean,
                                                   float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal,
                                                   int qk_gran, int blkq, int warpq, float sm_scale, int logit_mult_is_one,
                                                   const int32_t* block_lists, int64_t block_lists_bytes,
                                                   sage_stream_t stream) {
  AttnArgs a = int8_f8_args(q8, k8, v_fp8, o, o_dtype, q_scale, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                            qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  block_sparse(a, block_lists, block_lists_bytes);
  return run_attn(a, stream);
}

extern "C" int sage_attn_fusedq_pv_f16_blocksparse(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                   const sage_tensor* v, int v_dtype, const sage_tensor* o, int o_dtype,
                                                   const float* k_scale, const void* km, const float* v_mean, float* lse,
                                                   int B, int Hq, int Hk, int M, int N, int D, int is_causal, int qk_gran,
                                                   int warpq, float sm_scale, const int32_t* block_lists,
                                                   int64_t block_lists_bytes, sage_stream_t stream) {
  int status;
  AttnArgs a = fusedq_f16_args(status, q, q_dtype, k8, v, v_dtype, o, o_dtype, k_scale, km, v_mean, lse, B, Hq, Hk, M, N, D,
                               is_causal, qk_gran, warpq, sm_scale);
  if (status) return status;
  block_sparse(a, block_lists, block_lists_bytes);
  return run_attn(a, stream);
}

extern "C" int sage_attn_fusedq_pv_f8_blocksparse(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                  const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                                  const float* k_scale, const void* km, const float* v_scale,
                                                  const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N,
                                                  int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                                                  const int32_t* block_lists, int64_t block_lists_bytes,
                                                  sage_stream_t stream) {
  int status;
  AttnArgs a = fusedq_f8_args(status, q, q_dtype, k8, v_fp8, o, o_dtype, k_scale, km, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                              is_causal, qk_gran, warpq, sm_scale);
  if (status) return status;
  block_sparse(a, block_lists, block_lists_bytes);
  return run_attn(a, stream);
}

// ---- ... with the P.V skip: the block-sparse twins' arguments, then the per-head thresholds and the skip counters
extern "C" int sage_attn_qk_int8_pv_f16_blocksparse_pvskip(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v,
                                                           int v_dtype, const sage_tensor* o, int o_dtype,
                                                           const float* q_scale, const float* k_scale, const float* v_mean,
                                                           float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                                           int is_causal, int qk_gran, int blkq, int warpq, float sm_scale,
                                                           int logit_mult_is_one, const int32_t* block_lists,
                                                           int64_t block_lists_bytes, const float* pv_thresh,
                                                           int32_t* skipped, sage_stream_t stream) {
  AttnArgs a = int8_f16_args(q8, k8, v, v_dtype, o, o_dtype, q_scale, k_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                             qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  block_sparse(a, block_lists, block_lists_bytes);
  pv_skip(a, pv_thresh, skipped);
  return run_attn(a, stream);
}

extern "C" int sage_attn_qk_int8_pv_f8_blocksparse_pvskip(const sage_tensor* q8, const sage_tensor* k8,
                                                          const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                                          const float* q_scale, const float* k_scale, const float* v_scale,
                                                          const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                                          int N, int D, int is_causal, int qk_gran, int blkq, int warpq,
                                                          float sm_scale, int logit_mult_is_one, const int32_t* block_lists,
                                                          int64_t block_lists_bytes, const float* pv_thresh, int32_t* skipped,
                                                          sage_stream_t stream) {
  AttnArgs a = int8_f8_args(q8, k8, v_fp8, o, o_dtype, q_scale, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                            qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  block_sparse(a, block_lists, block_lists_bytes);
  pv_skip(a, pv_thresh, skipped);
  return run_attn(a, stream);
}

extern "C" int sage_attn_fusedq_pv_f16_blocksparse_pvskip(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                          const sage_tensor* v, int v_dtype, const sage_tensor* o,
                                                          int o_dtype, const float* k_scale, const void* km,
                                                          const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                                          int N, int D, int is_causal, int qk_gran, int warpq,
                                                          float sm_scale, const int32_t* block_lists,
                                                          int64_t block_lists_bytes, const float* pv_thresh, int32_t* skipped,
                                                          sage_stream_t stream) {
  int status;
  AttnArgs a = fusedq_f16_args(status, q, q_dtype, k8, v, v_dtype, o, o_dtype, k_scale, km, v_mean, lse, B, Hq, Hk, M, N, D,
                               is_causal, qk_gran, warpq, sm_scale);
  if (status) return status;
  block_sparse(a, block_lists, block_lists_bytes);
  pv_skip(a, pv_thresh, skipped);
  return run_attn(a, stream);
}

extern "C" int sage_attn_fusedq_pv_f8_blocksparse_pvskip(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                         const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                                         const float* k_scale, const void* km, const float* v_scale,
                                                         const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                                         int N, int D, int is_causal, int qk_gran, int warpq,
                                                         float sm_scale, const int32_t* block_lists,
                                                         int64_t block_lists_bytes, const float* pv_thresh, int32_t* skipped,
                                                         sage_stream_t stream) {
  int status;
  AttnArgs a = fusedq_f8_args(status, q, q_dtype, k8, v_fp8, o, o_dtype, k_scale, km, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                              is_causal, qk_gran, warpq, sm_scale);
  if (status) return status;
  block_sparse(a, block_lists, block_lists_bytes);
  pv_skip(a, pv_thresh, skipped);
  return run_attn(a, stream);
}

// ---- per-batch key lengths: the dense twins' arguments, then kv_lens
extern "C" int sage_attn_qk_int8_pv_f16_kvlen(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                              const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                              const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                              int is_causal, int qk_gran, int blkq, int warpq, float sm_scale,
                                              int logit_mult_is_one, const int32_t* kv_lens, sage_stream_t stream) {
  AttnArgs a = int8_f16_args(q8, k8, v, v_dtype, o, o_dtype, q_scale, k_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                             qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  key_lens(a, kv_lens);
  return run_attn(a, stream);
}

extern "C" int sage_attn_qk_int8_pv_f8_kvlen(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                             const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                             const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk,
                                             int M, int N, int D, int is_causal, int qk_gran, int blkq, int warpq,
                                             float sm_scale, int logit_mult_is_one, const int32_t* kv_lens,
                                             sage_stream_t stream) {
  AttnArgs a = int8_f8_args(q8, k8, v_fp8, o, o_dtype, q_scale, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                            qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  key_lens(a, kv_lens);
  return run_attn(a, stream);
}

extern "C" int sage_attn_fusedq_pv_f16_kvlen(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v,
                                             int v_dtype, const sage_tensor* o, int o_dtype, const float* k_scale,
                                             const void* km, const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                             int N, int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                                             const int32_t* kv_lens, sage_stream_t stream) {
  int status;
  AttnArgs a = fusedq_f16_args(status, q, q_dtype, k8, v, v_dtype, o, o_dtype, k_scale, km, v_mean, lse, B, Hq, Hk, M, N, D,
                               is_causal, qk_gran, warpq, sm_scale);
  if (status) return status;
  key_lens(a, kv_lens);
  return run_attn(a, stream);
}

extern "C" int sage_attn_fusedq_pv_f8_kvlen(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_fp8,
                                            const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                            const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk,
                                            int M, int N, int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                                            const int32_t* kv_lens, sage_stream_t stream) {
  int status;
  AttnArgs a = fusedq_f8_args(status, q, q_dtype, k8, v_fp8, o, o_dtype, k_scale, km, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                              is_causal, qk_gran, warpq, sm_scale);
  if (status) return status;
  key_lens(a, kv_lens);
  return run_attn(a, stream);
}

// ---- block-sparse attention with per-batch key lengths: the _blocksparse_pvskip twins' arguments, then kv_lens; a NULL
//      pv_thresh selects the kernel without the P.V skip (skipped is then not read)
extern "C" int sage_attn_qk_int8_pv_f16_blocksparse_kvlen(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v,
                                                          int v_dtype, const sage_tensor* o, int o_dtype, const float* q_scale,
                                                          const float* k_scale, const float* v_mean, float* lse, int B, int Hq,
                                                          int Hk, int M, int N, int D, int is_causal, int qk_gran, int blkq,
                                                          int warpq, float sm_scale, int logit_mult_is_one,
                                                          const int32_t* block_lists, int64_t block_lists_bytes,
                                                          const float* pv_thresh, int32_t* skipped, const int32_t* kv_lens,
                                                          sage_stream_t stream) {
  AttnArgs a = int8_f16_args(q8, k8, v, v_dtype, o, o_dtype, q_scale, k_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                             qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  block_sparse_key_lens(a, block_lists, block_lists_bytes, pv_thresh, skipped, kv_lens);
  return run_attn(a, stream);
}

extern "C" int sage_attn_qk_int8_pv_f8_blocksparse_kvlen(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                                         const sage_tensor* o, int o_dtype, const float* q_scale,
                                                         const float* k_scale, const float* v_scale, const float* v_mean,
                                                         float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal,
                                                         int qk_gran, int blkq, int warpq, float sm_scale,
                                                         int logit_mult_is_one, const int32_t* block_lists,
                                                         int64_t block_lists_bytes, const float* pv_thresh, int32_t* skipped,
                                                         const int32_t* kv_lens, sage_stream_t stream) {
  AttnArgs a = int8_f8_args(q8, k8, v_fp8, o, o_dtype, q_scale, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                            qk_gran, blkq, warpq, sm_scale, logit_mult_is_one);
  block_sparse_key_lens(a, block_lists, block_lists_bytes, pv_thresh, skipped, kv_lens);
  return run_attn(a, stream);
}

extern "C" int sage_attn_fusedq_pv_f16_blocksparse_kvlen(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                         const sage_tensor* v, int v_dtype, const sage_tensor* o, int o_dtype,
                                                         const float* k_scale, const void* km, const float* v_mean, float* lse,
                                                         int B, int Hq, int Hk, int M, int N, int D, int is_causal, int qk_gran,
                                                         int warpq, float sm_scale, const int32_t* block_lists,
                                                         int64_t block_lists_bytes, const float* pv_thresh, int32_t* skipped,
                                                         const int32_t* kv_lens, sage_stream_t stream) {
  int status;
  AttnArgs a = fusedq_f16_args(status, q, q_dtype, k8, v, v_dtype, o, o_dtype, k_scale, km, v_mean, lse, B, Hq, Hk, M, N, D,
                               is_causal, qk_gran, warpq, sm_scale);
  if (status) return status;
  block_sparse_key_lens(a, block_lists, block_lists_bytes, pv_thresh, skipped, kv_lens);
  return run_attn(a, stream);
}

extern "C" int sage_attn_fusedq_pv_f8_blocksparse_kvlen(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                        const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                                        const float* k_scale, const void* km, const float* v_scale,
                                                        const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N,
                                                        int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                                                        const int32_t* block_lists, int64_t block_lists_bytes,
                                                        const float* pv_thresh, int32_t* skipped, const int32_t* kv_lens,
                                                        sage_stream_t stream) {
  int status;
  AttnArgs a = fusedq_f8_args(status, q, q_dtype, k8, v_fp8, o, o_dtype, k_scale, km, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                              is_causal, qk_gran, warpq, sm_scale);
  if (status) return status;
  block_sparse_key_lens(a, block_lists, block_lists_bytes, pv_thresh, skipped, kv_lens);
  return run_attn(a, stream);
}
