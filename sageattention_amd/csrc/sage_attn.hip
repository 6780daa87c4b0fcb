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
#include "sage_entry.h"

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
  constexpr bool SPARSE = false, PVSKIP = false;
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
  constexpr bool CAUSAL = false, HAS_MASK = false, SPARSE = true, PVSKIP = false;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// (attn_i8_blocksparse_pvskip_kernel, the twin with SpargeAttn's second stage -- PVSKIP = true -- is built from the same body
//  in sage_attn_pvskip.hip: a file of its own because it needs a compiler option of its own, see there)

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

// block-sparse form: 4 waves, non-causal, no attn_mask
template <int D>
static int launch_blocksparse(const AttnCall& c, hipStream_t st) {
  const AttnParams& p = c.p;
  if (c.pvskip) {  // the twin with the P.V skip, then the same empty-row launch (which also zeroes the counters of its rows)
    if (const int s = launch_blocksparse_pvskip(c, st)) return s;
    hipLaunchKernelGGL(attn_blocksparse_empty_kernel, dim3(p.nqb * p.Hq * p.B), dim3(256), 0, st, p, c.D);
    return launch_status();
  }
  return by_flag(c.pv_fp8, [&](auto fp8) {
    constexpr bool PV_FP8 = decltype(fp8)::value;
    const size_t smem = (size_t)attn_ring_slots(D, 4, PV_FP8) * (64 * D + (PV_FP8 ? 64 * D : 64 * D * 2));
    return by_flag(c.kthread, [&](auto k) {
      return by_flag(!PV_FP8 && c.v_bf16, [&](auto v) {
        constexpr bool V_BF16 = !PV_FP8 && decltype(v)::value;
        auto kern = attn_i8_blocksparse_kernel<D, decltype(k)::value, V_BF16, PV_FP8>;
        if (!allow_lds((const void*)kern, smem)) return (int)SAGE_ERR_LAUNCH;
        hipLaunchKernelGGL(kern, dim3(p.nqb * p.Hq * p.B), dim3(256), smem, st, p);
        hipLaunchKernelGGL(attn_blocksparse_empty_kernel, dim3(p.nqb * p.Hq * p.B), dim3(256), 0, st, p, D);
        return launch_status();
      });
    });
  });
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
        const size_t smem = 2 * 64 * D + 2 * 64 * D * 2;
        return by_flag(c.kthread, [&](auto k) {
          return by_v([&](auto v) {
            return launch_kernel<D, NWAVES, false, decltype(k)::value, decltype(v)::value, false, true>(p, smem, st);
          });
        });
      }
    }
    const size_t smem = (size_t)attn_ring_slots(D, NWAVES, PV_FP8) * (64 * D + (PV_FP8 ? 64 * D : 64 * D * 2));  // RING x (K tile + V tile)
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
int attn_check(AttnCall& c, const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, bool pv_fp8, int v_dtype,
               const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale, const float* v_scale,
               const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal, int qk_gran,
               int blkq, int warpq, float sm_scale, int logit_mult_is_one, const AttnOptions& opt) {
  const int* const cu_q = opt.cu_q;
  const int* const cu_k = opt.cu_k;
  const int q_dtype = opt.q_dtype;
  const void* const km = opt.km;
  const void* const mask = opt.mask;
  const sage_kv_layout* const kvl = opt.kvl;
  const bool sparse = opt.block_sparse;
  if (sparse) {  // a block map combines with none of the other forms; its lists are read 16 bytes aligned rows
    if (!opt.block_lists || !aligned16(opt.block_lists)) return SAGE_ERR_INVALID_ARGUMENT;
    if (opt.pv_skip && (!opt.pv_thresh || ((uintptr_t)opt.pv_thresh & 3) || ((uintptr_t)opt.pv_skipped & 3)))
      return SAGE_ERR_INVALID_ARGUMENT;
    if (is_causal || cu_q || cu_k || mask || kvl || v_mean) return SAGE_ERR_UNSUPPORTED;
  }
  if (mask && (opt.mask_kind < 1 || opt.mask_kind > 3 || !opt.mask_strides || is_causal || pv_fp8 || cu_q)) return SAGE_ERR_INVALID_ARGUMENT;
  const bool fusedq = q_dtype >= 0;  // q8 is then the fp16/bf16 query tensor
  if ((cu_q == nullptr) != (cu_k == nullptr)) return SAGE_ERR_INVALID_ARGUMENT;
  if (fusedq) {
    if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
    if (qk_gran == SAGE_GRAN_PER_BLOCK || cu_q || (km && !aligned16(km))) return SAGE_ERR_UNSUPPORTED;
    if (!tensor_ok(q8, 8) || !k_scale) return SAGE_ERR_INVALID_ARGUMENT;
    q_scale = k_scale;  // unused placeholder so the shared checks below pass
  }
  if (cu_q && (pv_fp8 || lse)) return SAGE_ERR_UNSUPPORTED;  // packed sequences: fp16 PV, no LSE (as the reference)
  if (!tensor_ok(q8, fusedq ? 8 : 16) || !tensor_ok(k8, 16) || !tensor_ok(v, pv_fp8 ? 16 : 8) || !tensor_ok(o, 4) || !q_scale ||
      !k_scale)
    return SAGE_ERR_INVALID_ARGUMENT;
  if (pv_fp8 && !v_scale) return SAGE_ERR_INVALID_ARGUMENT;
  if (B <= 0 || Hq <= 0 || Hk <= 0 || M <= 0 || N <= 0 || Hq % Hk != 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (sparse && opt.block_lists_bytes < block_sparse_bytes(B, Hq, M, N)) return SAGE_ERR_INVALID_ARGUMENT;
  // the integer row max and the -inf mask pattern rely on a positive, finite dequantisation scale
  if (!logit_mult_is_one && !(sm_scale > 0.f && sm_scale < 1.0e30f)) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = dim_dtype_status(D, v_dtype)) return s;
  if (o_dtype != SAGE_F16 && o_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  if (qk_gran < SAGE_GRAN_PER_BLOCK || qk_gran > SAGE_GRAN_PER_THREAD) return SAGE_ERR_INVALID_ARGUMENT;
  if (blkq != 64 && blkq != 128) return SAGE_ERR_INVALID_ARGUMENT;
  if (qk_gran == SAGE_GRAN_PER_BLOCK) warpq = blkq;
  if ((warpq != 16 && warpq != 32 && warpq != 64 && warpq != 128) || blkq % warpq != 0) return SAGE_ERR_INVALID_ARGUMENT;
  if ((v_mean && !aligned16(v_mean)) || (v_scale && !aligned16(v_scale))) return SAGE_ERR_INVALID_ARGUMENT;
  // KV tile layout: dense by default (a tile = 64 consecutive rows of the sage_tensor), explicit for tile-major buffers
  const int64_t ntile = ((int64_t)N + 63) >> 6;
  int64_t k_tile = 64 * k8->stride_n, v_tile = pv_fp8 ? 64 : 128 * v->stride_n;  // bytes
  const int per_tile = qk_gran == SAGE_GRAN_PER_THREAD ? 4 : 1;
  int64_t ks_h = ntile * per_tile, ks_b = ks_h * Hk, ks_t = per_tile;
  bool tiled = false;
  if (kvl) {
    if (cu_q || mask || kvl->k_tile_stride < 0 || kvl->v_tile_stride < 0) return SAGE_ERR_INVALID_ARGUMENT;
    if (kvl->k_tile_stride) { k_tile = kvl->k_tile_stride; tiled = true; }
    if (kvl->v_tile_stride) { v_tile = pv_fp8 ? kvl->v_tile_stride : 2 * kvl->v_tile_stride; tiled = true; }
    if (kvl->ks_stride_b || kvl->ks_stride_h || kvl->ks_stride_tile) {
      if (kvl->ks_stride_tile < per_tile || kvl->ks_stride_h < 0 || kvl->ks_stride_b < 0) return SAGE_ERR_INVALID_ARGUMENT;
      ks_b = kvl->ks_stride_b; ks_h = kvl->ks_stride_h; ks_t = kvl->ks_stride_tile;
      if (per_tile == 4 && ((ks_b | ks_h | ks_t) & 3)) return SAGE_ERR_INVALID_ARGUMENT;  // 16-B scalar loads
    }
    if ((k_tile & 15) || (v_tile & 15)) return SAGE_ERR_INVALID_ARGUMENT;
  }
  // the K/V slices of one (b, h_kv) are addressed with 32-bit buffer offsets
  const int64_t lim = (int64_t)1 << 31;
  if (ntile * k_tile + 64 * k8->stride_n + D >= lim) return SAGE_ERR_TOO_LARGE;
  if (pv_fp8 ? (ntile * v_tile + (int64_t)D * v->stride_n + 64 >= lim) : (ntile * v_tile + (64 * v->stride_n + D) * 2 >= lim)) return SAGE_ERR_TOO_LARGE;
  if (ks_t * ntile >= lim) return SAGE_ERR_TOO_LARGE;
  AttnParams& p = c.p;
  p.q = (const int8_t*)q8->data; p.qsb = q8->stride_b; p.qsh = q8->stride_h; p.qsn = q8->stride_n;
  p.k = (const int8_t*)k8->data; p.ksb = k8->stride_b; p.ksh = k8->stride_h; p.ksn = k8->stride_n;
  p.v = (const uint8_t*)v->data; p.vsb = v->stride_b; p.vsh = v->stride_h; p.vsn = v->stride_n;
  p.o = (uint16_t*)o->data; p.osb = o->stride_b; p.osh = o->stride_h; p.osn = o->stride_n;
  p.q_scale = q_scale; p.k_scale = k_scale; p.v_scale = v_scale; p.v_mean = v_mean; p.lse = lse;
  p.B = B; p.Hq = Hq; p.Hk = Hk; p.M = M; p.N = N;
  const int nblkq = (M + blkq - 1) / blkq;
  p.gq = qk_gran == SAGE_GRAN_PER_BLOCK ? nblkq : qk_gran == SAGE_GRAN_PER_WARP ? nblkq * (blkq / warpq) : nblkq * (blkq / warpq) * 8;
  const int nblkk = (N + 63) / 64;
  p.gk = qk_gran == SAGE_GRAN_PER_THREAD ? nblkk * 4 : nblkk;
  p.qgran = qk_gran; p.blkq = blkq; p.warpq = warpq;
  p.logit_mult = logit_mult_is_one ? 1.0f : sm_scale * kLog2e;
  p.out_bf16 = o_dtype == SAGE_BF16;
  p.cu_q = cu_q; p.cu_k = cu_k;
  p.mask = (const uint8_t*)mask; p.mask_kind = mask ? opt.mask_kind : 0;
  const int64_t* const ms = opt.mask_strides;
  p.msb = mask ? ms[0] : 0; p.msh = mask ? ms[1] : 0; p.msm = mask ? ms[2] : 0; p.msn = mask ? ms[3] : 0;
  p.k_tile_bytes = (int)k_tile; p.v_tile_bytes = (int)v_tile; p.ks_b = ks_b; p.ks_h = ks_h; p.ks_t = (int)ks_t;
  p.kv_tiled = tiled ? 1 : 0;
  p.o_vec16 = (o->stride_b % 8 == 0 && o->stride_h % 8 == 0 && o->stride_n % 8 == 0) ? 1 : 0;  // 16-byte aligned output rows
  p.q_f16 = fusedq ? (const uint16_t*)q8->data : nullptr;
  p.km = (const uint16_t*)km; p.q_bf16 = q_dtype == SAGE_BF16; p.sm_scale = sm_scale;
  // measured on MI355X: D=128 fp16 PV -> one 8-wave workgroup per CU (4-wave: -3 %); D=128 fp8 PV -> two 4-wave
  // workgroups per CU (+3.6 % non-causal, +5.7 % causal); D=64 (<= 168 VGPRs) -> 4-wave workgroups, 3 per CU
  // ... except for short key sequences (few tiles per workgroup, so prologue and epilogue weigh more and two smaller
  // workgroups per CU overlap them better): end to end, 4-wave 0.959x the 8-wave time at 2048 keys, 0.979x at 3072, 0.998x
  // at 4096, 1.02x from 6144; causal 0.993x at 8192 (4096 keys per row on average) -> 4 waves up to 3072 keys per row
  // (profiles/r03_ab/geometry_end_to_end.log).
  const int keys_per_row = is_causal ? N / 2 : N;
  // FP8 PV at head_dim 128: 4-wave workgroups +2.2 % at 8K keys, +0.7 % at 16K, -1.1 % at 32K, -1.3 % at 64K.  The two
  // co-resident 4-wave workgroups of a CU drift apart on a long stream until they no longer share K/V tiles in L2 (1.90x the
  // algorithmic HBM-side bytes with 4 waves, 1.00x with 8: profiles/r03_ab/fetch_by_geometry.md) -> 8 waves beyond 24K keys per row.
  // (block-sparse: always 4 waves -- a workgroup is one block row of the map; the tuning knobs do not apply)
  const int nw = sparse                ? 4
                 : opt.nwaves          ? opt.nwaves
                 : g_nwaves_override ? g_nwaves_override
                                     : ((D == 64 || (pv_fp8 && keys_per_row <= 24576) || keys_per_row <= 3072) ? 4 : 8);
  p.nqb = (M + nw * 32 - 1) / (nw * 32);
  if (sparse) { p.bs_lists = opt.block_lists; p.bs_row = (int)block_list_row(N); }  // (share the words of mask / mask_kind)
  c.pvskip = sparse && opt.pv_skip;
  if (c.pvskip) { p.pv_thresh = opt.pv_thresh; p.pv_skipped = opt.pv_skipped; }  // (... and those of two mask strides)
  c.D = D; c.nwaves = nw; c.sparse = sparse;
  c.pv_fp8 = pv_fp8; c.causal = is_causal != 0; c.kthread = qk_gran == SAGE_GRAN_PER_THREAD; c.v_bf16 = v_dtype == SAGE_BF16;
  return SAGE_OK;
}

int attn_launch(const AttnCall& c, hipStream_t st) {
  return by_dim(c.D, [&](auto d) {
    if (c.sparse) return launch_blocksparse<decltype(d)::value>(c, st);
    return c.nwaves == 8 ? launch_attn<decltype(d)::value, 8>(c, st) : launch_attn<decltype(d)::value, 4>(c, st);
  });
}

// the public entry points: check, then launch
static int run_attn(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, bool pv_fp8, int v_dtype,
                    const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale, const float* v_scale,
                    const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal, int qk_gran,
                    int blkq, int warpq, float sm_scale, int logit_mult_is_one, sage_stream_t stream,
                    const AttnOptions& opt = AttnOptions()) {
  AttnCall c;
  if (const int s = attn_check(c, q8, k8, v, pv_fp8, v_dtype, o, o_dtype, q_scale, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M,
                               N, D, is_causal, qk_gran, blkq, warpq, sm_scale, logit_mult_is_one, opt))
    return s;
  return attn_launch(c, (hipStream_t)stream);
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
  return run_attn(q8, k8, v, false, v_dtype, o, o_dtype, q_scale, k_scale, nullptr, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                  qk_gran, blkq, warpq, sm_scale, logit_mult_is_one, stream);
}

extern "C" int sage_attn_qk_int8_pv_f8(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                       const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                       const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                       int N, int D, int is_causal, int qk_gran, int blkq, int warpq, float sm_scale,
                                       int logit_mult_is_one, sage_stream_t stream) {
  return run_attn(q8, k8, v_fp8, true, SAGE_F16, o, o_dtype, q_scale, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                  is_causal, qk_gran, blkq, warpq, sm_scale, logit_mult_is_one, stream);
}

extern "C" int sage_attn_qk_int8_pv_f16_varlen(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                               const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                               const int* cu_seqlens_q, const int* cu_seqlens_k, int num_seqs, int Hq, int Hk,
                                               int max_seqlen_q, int max_seqlen_k, int D, int is_causal, int qk_gran, int blkq,
                                               int warpq, float sm_scale, int logit_mult_is_one, sage_stream_t stream) {
  if (!cu_seqlens_q || !cu_seqlens_k) return SAGE_ERR_INVALID_ARGUMENT;
  AttnOptions opt;
  opt.cu_q = cu_seqlens_q;
  opt.cu_k = cu_seqlens_k;
  return run_attn(q8, k8, v, false, v_dtype, o, o_dtype, q_scale, k_scale, nullptr, nullptr, nullptr, num_seqs, Hq, Hk,
                  max_seqlen_q, max_seqlen_k, D, is_causal, qk_gran, blkq, warpq, sm_scale, logit_mult_is_one,
                  stream, opt);
}

extern "C" int sage_attn_fusedq_pv_f16(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                       const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                       const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                       int is_causal, int qk_gran, int warpq, float sm_scale, sage_stream_t stream) {
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  AttnOptions opt;
  opt.q_dtype = q_dtype;
  opt.km = km;
  return run_attn(q, k8, v, false, v_dtype, o, o_dtype, nullptr, k_scale, nullptr, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                  qk_gran, 128, warpq, sm_scale, 0, stream, opt);
}

extern "C" int sage_attn_fusedq_pv_f8(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_fp8,
                                      const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                      const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                      int N, int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                                      sage_stream_t stream) {
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  AttnOptions opt;
  opt.q_dtype = q_dtype;
  opt.km = km;
  return run_attn(q, k8, v_fp8, true, SAGE_F16, o, o_dtype, nullptr, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                  is_causal, qk_gran, 128, warpq, sm_scale, 0, stream, opt);
}

extern "C" int sage_attn_qk_int8_pv_f16_masked(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                               const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                               const void* attn_mask, int mask_kind, const int64_t* mask_strides, float* lse,
                                               int B, int Hq, int Hk, int M, int N, int D, int qk_gran, int blkq, int warpq,
                                               float sm_scale, int logit_mult_is_one, sage_stream_t stream) {
  if (!attn_mask) return SAGE_ERR_INVALID_ARGUMENT;
  AttnOptions opt;
  opt.mask = attn_mask;
  opt.mask_kind = mask_kind;
  opt.mask_strides = mask_strides;
  return run_attn(q8, k8, v, false, v_dtype, o, o_dtype, q_scale, k_scale, nullptr, nullptr, lse, B, Hq, Hk, M, N, D, 0, qk_gran,
                  blkq, warpq, sm_scale, logit_mult_is_one, stream, opt);
}

extern "C" int sage_attn_qk_int8_pv_f16_kvtiles(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                                const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                                const sage_kv_layout* kv_layout, float* lse, int B, int Hq, int Hk, int M,
                                                int N, int D, int is_causal, int qk_gran, int blkq, int warpq, float sm_scale,
                                                sage_stream_t stream) {
  if (!kv_layout) return SAGE_ERR_INVALID_ARGUMENT;
  AttnOptions opt;
  opt.kvl = kv_layout;
  return run_attn(q8, k8, v, false, v_dtype, o, o_dtype, q_scale, k_scale, nullptr, nullptr, lse, B, Hq, Hk, M, N, D, is_causal,
                  qk_gran, blkq, warpq, sm_scale, 0, stream, opt);
}

extern "C" int sage_attn_qk_int8_pv_f8_kvtiles(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                               const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                               const float* v_scale, const sage_kv_layout* kv_layout, float* lse, int B,
                                               int Hq, int Hk, int M, int N, int D, int is_causal, int qk_gran, int blkq,
                                               int warpq, float sm_scale, sage_stream_t stream) {
  if (!kv_layout) return SAGE_ERR_INVALID_ARGUMENT;
  AttnOptions opt;
  opt.kvl = kv_layout;
  return run_attn(q8, k8, v_fp8, true, SAGE_F16, o, o_dtype, q_scale, k_scale, v_scale, nullptr, lse, B, Hq, Hk, M, N, D,
                  is_causal, qk_gran, blkq, warpq, sm_scale, 0, stream, opt);
}

// ---- block-sparse forms: the dense twins' arguments plus the tile lists of sage_block_map_compact
static AttnOptions blocksparse_options(const int32_t* block_lists, int64_t block_lists_bytes) {
  AttnOptions opt;
  opt.block_sparse = true;
  opt.block_lists = block_lists;
  opt.block_lists_bytes = block_lists_bytes;
  return opt;
}

extern "C" int sage_attn_qk_int8_pv_f16_blocksparse(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v,
                                                    int v_dtype, const sage_tensor* o, int o_dtype, const float* q_scale,
                                                    const float* k_scale, const float* v_mean, float* lse, int B, int Hq,
                                                    int Hk, int M, int N, int D, int is_causal, int qk_gran, int blkq,
                                                    int warpq, float sm_scale, int logit_mult_is_one,
                                                    const int32_t* block_lists, int64_t block_lists_bytes,
                                                    sage_stream_t stream) {
  return run_attn(q8, k8, v, false, v_dtype, o, o_dtype, q_scale, k_scale, nullptr, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                  qk_gran, blkq, warpq, sm_scale, logit_mult_is_one, stream, blocksparse_options(block_lists, block_lists_bytes));
}

extern "C" int sage_attn_qk_int8_pv_f8_blocksparse(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                                   const sage_tensor* o, int o_dtype, const float* q_scale,
                                                   const float* k_scale, const float* v_scale, const float* v_mean,
                                                   float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal,
                                                   int qk_gran, int blkq, int warpq, float sm_scale, int logit_mult_is_one,
                                                   const int32_t* block_lists, int64_t block_lists_bytes,
                                                   sage_stream_t stream) {
  return run_attn(q8, k8, v_fp8, true, SAGE_F16, o, o_dtype, q_scale, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                  is_causal, qk_gran, blkq, warpq, sm_scale, logit_mult_is_one, stream,
                  blocksparse_options(block_lists, block_lists_bytes));
}

extern "C" int sage_attn_fusedq_pv_f16_blocksparse(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                   const sage_tensor* v, int v_dtype, const sage_tensor* o, int o_dtype,
                                                   const float* k_scale, const void* km, const float* v_mean, float* lse,
                                                   int B, int Hq, int Hk, int M, int N, int D, int is_causal, int qk_gran,
                                                   int warpq, float sm_scale, const int32_t* block_lists,
                                                   int64_t block_lists_bytes, sage_stream_t stream) {
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  AttnOptions opt = blocksparse_options(block_lists, block_lists_bytes);
  opt.q_dtype = q_dtype;
  opt.km = km;
  return run_attn(q, k8, v, false, v_dtype, o, o_dtype, nullptr, k_scale, nullptr, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                  qk_gran, 128, warpq, sm_scale, 0, stream, opt);
}

extern "C" int sage_attn_fusedq_pv_f8_blocksparse(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                  const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                                  const float* k_scale, const void* km, const float* v_scale,
                                                  const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N,
                                                  int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                                                  const int32_t* block_lists, int64_t block_lists_bytes,
                                                  sage_stream_t stream) {
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  AttnOptions opt = blocksparse_options(block_lists, block_lists_bytes);
  opt.q_dtype = q_dtype;
  opt.km = km;
  return run_attn(q, k8, v_fp8, true, SAGE_F16, o, o_dtype, nullptr, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                  is_causal, qk_gran, 128, warpq, sm_scale, 0, stream, opt);
}

// ---- ... with the P.V skip: the block-sparse twins' arguments, then the per-head thresholds and the skip counters
static AttnOptions pvskip_options(const int32_t* block_lists, int64_t block_lists_bytes, const float* pv_thresh,
                                  int32_t* skipped) {
  AttnOptions opt = blocksparse_options(block_lists, block_lists_bytes);
  opt.pv_skip = true;
  opt.pv_thresh = pv_thresh;
  opt.pv_skipped = skipped;
  return opt;
}

extern "C" int sage_attn_qk_int8_pv_f16_blocksparse_pvskip(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v,
                                                           int v_dtype, const sage_tensor* o, int o_dtype,
                                                           const float* q_scale, const float* k_scale, const float* v_mean,
                                                           float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                                           int is_causal, int qk_gran, int blkq, int warpq, float sm_scale,
                                                           int logit_mult_is_one, const int32_t* block_lists,
                                                           int64_t block_lists_bytes, const float* pv_thresh,
                                                           int32_t* skipped, sage_stream_t stream) {
  return run_attn(q8, k8, v, false, v_dtype, o, o_dtype, q_scale, k_scale, nullptr, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                  qk_gran, blkq, warpq, sm_scale, logit_mult_is_one, stream,
                  pvskip_options(block_lists, block_lists_bytes, pv_thresh, skipped));
}

extern "C" int sage_attn_qk_int8_pv_f8_blocksparse_pvskip(const sage_tensor* q8, const sage_tensor* k8,
                                                          const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                                          const float* q_scale, const float* k_scale, const float* v_scale,
                                                          const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                                          int N, int D, int is_causal, int qk_gran, int blkq, int warpq,
                                                          float sm_scale, int logit_mult_is_one, const int32_t* block_lists,
                                                          int64_t block_lists_bytes, const float* pv_thresh, int32_t* skipped,
                                                          sage_stream_t stream) {
  return run_attn(q8, k8, v_fp8, true, SAGE_F16, o, o_dtype, q_scale, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                  is_causal, qk_gran, blkq, warpq, sm_scale, logit_mult_is_one, stream,
                  pvskip_options(block_lists, block_lists_bytes, pv_thresh, skipped));
}

extern "C" int sage_attn_fusedq_pv_f16_blocksparse_pvskip(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                          const sage_tensor* v, int v_dtype, const sage_tensor* o,
                                                          int o_dtype, const float* k_scale, const void* km,
                                                          const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                                          int N, int D, int is_causal, int qk_gran, int warpq,
                                                          float sm_scale, const int32_t* block_lists,
                                                          int64_t block_lists_bytes, const float* pv_thresh, int32_t* skipped,
                                                          sage_stream_t stream) {
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  AttnOptions opt = pvskip_options(block_lists, block_lists_bytes, pv_thresh, skipped);
  opt.q_dtype = q_dtype;
  opt.km = km;
  return run_attn(q, k8, v, false, v_dtype, o, o_dtype, nullptr, k_scale, nullptr, v_mean, lse, B, Hq, Hk, M, N, D, is_causal,
                  qk_gran, 128, warpq, sm_scale, 0, stream, opt);
}

extern "C" int sage_attn_fusedq_pv_f8_blocksparse_pvskip(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                                         const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                                         const float* k_scale, const void* km, const float* v_scale,
                                                         const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                                         int N, int D, int is_causal, int qk_gran, int warpq,
                                                         float sm_scale, const int32_t* block_lists,
                                                         int64_t block_lists_bytes, const float* pv_thresh, int32_t* skipped,
                                                         sage_stream_t stream) {
  if (q_dtype != SAGE_F16 && q_dtype != SAGE_BF16) return SAGE_ERR_INVALID_ARGUMENT;
  AttnOptions opt = pvskip_options(block_lists, block_lists_bytes, pv_thresh, skipped);
  opt.q_dtype = q_dtype;
  opt.km = km;
  return run_attn(q, k8, v_fp8, true, SAGE_F16, o, o_dtype, nullptr, k_scale, v_scale, v_mean, lse, B, Hq, Hk, M, N, D,
                  is_causal, qk_gran, 128, warpq, sm_scale, 0, stream, opt);
}
