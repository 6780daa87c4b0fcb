/*
 * sageattn_hip.h -- C ABI of the MI355X (gfx950) native SageAttention hot path.
 *
 * Drop-in boundary for the path sageattn() / sageattn_qk_int8_pv_{fp16,fp8}_* of
 * eliotwang/SageAttention (sageattention/core.py:80-905).  Every entry point below replaces one
 * or more functions that the reference binds through pybind (module names
 * sageattention._fused and sageattention._qattn_{sm80,sm89,rocm}); the reference interface each
 * one replaces is cited as file:line of the reference tree.  INTEGRATION.md shows the
 * reference-side binding.
 *
 * Conventions
 *  - plain C: device pointers, sizes, element strides; no torch types.  All pointers are DEVICE
 *    pointers of the current HIP device unless stated otherwise.
 *  - tensors are 4-D [B,H,N,D] views with unit stride on D, described by sage_tensor (strides in
 *    ELEMENTS): this covers both reference layouts, tensor_layout 1 = "HND" [B,H,N,D] and
 *    0 = "NHD" [B,N,H,D] (core.py:585; strides selected as in qk_int_sv_f16_cuda_sm80.cu:728-764).
 *  - ownership as in the reference: the caller allocates every buffer, the callee
 *    keeps no state; work is enqueued on `stream` and never synchronised.
 *  - every function returns SAGE_OK (0) or a negative sage_status; nothing is printed, nothing
 *    aborts (the reference raises through TORCH_CHECK / std::invalid_argument, utils.cuh:20-38).
 *  - a call that returns an argument status (SAGE_ERR_INVALID_ARGUMENT, _UNSUPPORTED_HEAD_DIM,
 *    _UNSUPPORTED, _TOO_LARGE) has enqueued no work: every argument is checked before the first launch.
 */
#ifndef SAGEATTN_HIP_H
#define SAGEATTN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAGEATTN_HIP_ABI_VERSION 3

typedef void* sage_stream_t; /* hipStream_t */

typedef enum sage_status {
  SAGE_OK = 0,
  SAGE_ERR_INVALID_ARGUMENT = -1, /* bad enum / null pointer / inconsistent sizes          */
  SAGE_ERR_UNSUPPORTED_HEAD_DIM = -2, /* head_dim not in {64,128} (dispatch_utils.h:23-34)  */
  SAGE_ERR_UNSUPPORTED = -3,      /* valid in the reference, not built here                */
  SAGE_ERR_TOO_LARGE = -4,        /* a (b,h) slice exceeds the 2^31-byte buffer window       */
  SAGE_ERR_LAUNCH = -5            /* hipGetLastError() != hipSuccess after the launch       */
} sage_status;

typedef enum sage_dtype { SAGE_F16 = 0, SAGE_BF16 = 1 } sage_dtype;

/* csrc/qattn/attn_utils.cuh:49-54 (QuantGranularity); values cross the reference's pybind ABI as
 * ints (core.py:587: per_warp = 2, per_thread = 3). */
typedef enum sage_qk_gran {
  SAGE_GRAN_PER_BLOCK = 1,
  SAGE_GRAN_PER_WARP = 2,
  SAGE_GRAN_PER_THREAD = 3
} sage_qk_gran;

/* Quantizer numerics: the reference has two statements of the INT8 quantizer that differ in the
 * last bit. */
typedef enum sage_rounding {
  SAGE_ROUND_TRITON = 0, /* scale=amax/127 (+eps per-thread); q=trunc(x/scale + 0.5*sign);
                            mean subtracted in the input dtype  (triton/quant_per_block.py:39-54) */
  SAGE_ROUND_CUDA = 1    /* amax=max(1e-7,amax); q=rint_even(x*(127/amax)) saturated;
                            mean subtracted in fp32              (csrc/fused/fused.cu:119-184)    */
} sage_rounding;

typedef struct sage_tensor {
  void* data;
  int64_t stride_b, stride_h, stride_n; /* elements */
} sage_tensor;

/* ---- library ------------------------------------------------------------------------------ */
int sage_abi_version(void);
const char* sage_status_string(int status);
/* Compile-time target of the device code in this library ("gfx950"). */
const char* sage_target_arch(void);

/* Tuning knob of the CALLING HOST THREAD (speed only, never results): it applies to the attention launches this thread
 * makes afterwards and to no other thread's.  key SAGE_TUNE_NWAVES: waves per workgroup of the attention kernels, value
 * in {0 = the library's measured choice, 4, 8}.  The one-call operators (sage_sageattn_*) take the same choice per call
 * in their options struct instead. */
typedef enum sage_tune_key { SAGE_TUNE_NWAVES = 0 } sage_tune_key;
int sage_set_tuning(int key, int value);
int sage_get_tuning(int key); /* the calling thread's value; -1 for an unknown key */

/* ---- K smoothing ---------------------------------------------------------------------------
 * km[b,h,:] = mean over n of k[b,h,n,:], fp32 accumulation, one rounding to `dtype`.
 * Replaces the torch op `k.mean(dim=seq_dim, keepdim=True)` at core.py:612,794.
 * workspace: fp32, at least sage_k_mean_workspace_bytes(B,H,N,D) bytes (deterministic two-pass
 * reduction, no atomics).  km: [B,H,D] contiguous, same dtype as k. */
size_t sage_k_mean_workspace_bytes(int B, int H, int N, int D);
int sage_k_mean(const sage_tensor* k, int dtype, int B, int H, int N, int D,
                void* km, void* workspace, sage_stream_t stream);

/* ---- INT8 Q/K quantizer ---------------------------------------------------------------------
 * Replaces, by (gran, rounding, mean, mult):
 *   quant_per_block_int8_cuda (2 overloads)        csrc/fused/fused.cu:429-592, pybind.cpp:23-25
 *   quant_per_block_int8_fuse_sub_mean_cuda         csrc/fused/fused.cu:594-682
 *   quant_per_warp_int8_cuda                        csrc/fused/fused.cu:685-768
 *   triton per_block_int8 / per_thread_int8         sageattention/triton/quant_per_block.py:48,
 *                                                   sageattention/triton/quant_per_thread.py:158
 * x: [B,H,N,D] fp16/bf16;  out: int8 same logical shape;  scale: fp32 [B,H,G] contiguous with
 *   per_block : G = ceil(N/blk)                     one scale per blk rows
 *   per_warp  : G = ceil(N/blk)*(blk/warp)          one scale per warp rows
 *   per_thread: is_key=0: G = ceil(N/blk)*(blk/warp)*8, rows with equal r%8 inside a warp group
 *               is_key=1: G = ceil(N/blk)*(blk/warp)*4, rows with equal (r%8)/2
 * mean: optional [B,H,D] (same dtype as x, contiguous) subtracted before quantization (smooth_k).
 * mult: multiplied into x (fp32) before quantization (Q of the per-block path: sm_scale*log2e).
 * lse_dot/lse_dot_vec: optional; lse_dot[b,h,n] = sum_d x[b,h,n,d]*lse_dot_vec[b,h/dot_group,d]
 *   in fp32 (the `q @ km^T` LSE correction of core.py:613-617), fp32 [B,H,N] contiguous.
 * blk in {64,128}; warp in {16,32,64} and divides blk; D in {64,128}. */
int sage_quant_qk_int8(const sage_tensor* x, int dtype, int B, int H, int N, int D,
                       const void* mean, const sage_tensor* out, float* scale,
                       int gran, int is_key, int blk, int warp, float mult, int rounding,
                       const void* lse_dot_vec, int dot_group, float* lse_dot,
                       sage_stream_t stream);

/* ---- V smoothing for the fp16-accumulate path ---------------------------------------------------
 * out = fp16(v - vm) with vm [B,H,D] (dtype of v).  Replaces sub_mean_cuda, fused.cu:770-848. */
int sage_sub_mean_f16(const sage_tensor* v, int dtype, int B, int H, int N, int D,
                      const void* vm, const sage_tensor* out, sage_stream_t stream);

/* ---- FP8 V quantizer ------------------------------------------------------------------------
 * Replaces transpose_pad_permute_cuda + scale_fuse_quant_cuda / mean_scale_fuse_quant_cuda
 * (csrc/fused/fused.cu:850-1083, sageattention/quant.py:225-322) in one fused pair of kernels.
 * v: [B,H,N,D] fp16/bf16.  v_fp8: OCP e4m3fn bytes, logical [B,H,D,Npad] with Npad=ceil64(N),
 * described by (stride_b, stride_h, stride_n:=stride of the D index); zero beyond N.
 * v_scale[b,h,d] = amax_d/scale_max (fp32 [B,H,D]); v_mean (optional, fp32 [B,H,D]): when non
 * null the channel mean (sum/ceil16(N), fused.cu:335,381) is subtracted first.
 * A channel with amax_d == 0 (all zero over the sequence; every channel of a zero-padded head dim) is defined: its
 * image is all 0x00 and v_scale is 0, so the attention output of that channel is exactly 0.  The reference forms
 * scale_max/0 = inf and (0-0)*inf = NaN there (fused.cu:399); this is the only departure from it, and only where it
 * returns NaN.  The same holds for sage_kv_prepare_fp8(_kvlen) and sage_kv_stats_reduce.
 * The reference's 16-row permutation (quant.py:234) is an NVIDIA mma-fragment artefact and is
 * not applied (the fork's HIP port disables it too, fused.hip:362-367).  Its gfx950 counterpart IS:
 * inside every 64-token block position pos holds token
 *   32*((pos&31)>>4) + (pos&3) + 8*((pos&15)>>2) + 4*(pos>>5)
 * ("MFMA order": the k order in which v_mfma_scale_f32_32x32x64_f8f6f4 receives P^T out of the S^T
 * accumulators), so v_fp8 is an opaque operand of sage_attn_qk_int8_pv_f8.  Columns of tokens >= N
 * are zero.
 * workspace: sage_quant_v_fp8_workspace_bytes(B,H,N,D) bytes. */
size_t sage_quant_v_fp8_workspace_bytes(int B, int H, int N, int D);
int sage_quant_v_fp8(const sage_tensor* v, int dtype, int B, int H, int N, int D,
                     const sage_tensor* v_fp8, float* v_scale, float* v_mean, float scale_max,
                     void* workspace, sage_stream_t stream);

/* ---- fused attention, INT8 QK^T + FP16 PV ------------------------------------------------------
 * Replaces qk_int8_sv_f16_accum_f32_attn, qk_int8_sv_f16_accum_f16_attn,
 * qk_int8_sv_f16_accum_f16_attn_inst_buf, qk_int8_sv_f16_accum_f16_fuse_v_mean_attn
 * (csrc/qattn/attn_cuda_sm80.h:19-65, qk_int_sv_f16_cuda_sm80.cu:674-1379).  On gfx950 the PV
 * MFMA accumulates in fp32 for every pv_accum_dtype the reference names.
 *   q8 [B,Hq,M,D] int8, k8 [B,Hk,N,D] int8, v [B,Hk,N,D] fp16 or bf16 (v_dtype), o [B,Hq,M,D] fp16/bf16 (o_dtype).
 *   A bf16 v is used as it is: P is rounded to bf16 and P.V runs on the bf16 MFMA with fp32 accumulation (the reference
 *   converts v to fp16 first, core.py:633 `v.to(float16)`; a caller who wants exactly that passes the converted tensor).
 *   Precision note: v_dtype = BF16 selects the bf16 P (8 significant bits) whatever o_dtype is -- with o_dtype = F16 the
 *   result carries 3 bits less in P than the fp16-V call (|do| <= 2^-8 * sum(p |v|) / l per element); bf16 outputs round
 *   at that size anyway.
 *   q_scale / k_scale: fp32 [B,Hq,Gq] / [B,Hk,Gk] with the shapes sage_quant_qk_int8 produces for
 *   (gran, blkq, warpq, blkk=64, warpk=64)  (…sm80.cu:796-805).
 *   sm_scale: logits are multiplied by sm_scale*log2(e) inside the kernel (…sm80.cu:92); must be
 *   positive and finite (SAGE_ERR_INVALID_ARGUMENT otherwise: the integer row max and the masks
 *   assume a positive dequantisation scale).
 *   logit_mult_is_one != 0: the scales already contain sm_scale*log2e (triton per_block path,
 *   attn_qk_int8_per_block.py:47) and sm_scale is ignored.
 *   v_mean: optional fp32 [B,Hk,D] added to the output rows (fuse_v_mean).
 *   lse: optional fp32 [B,Hq,M]; receives log2-domain lse of the scaled, smoothed logits
 *   (…sm80.cu:657-668); the caller applies core.py:651.
 *   is_causal: kv_idx > q_idx masked (top-left aligned, attn_utils.cuh:296-323). */
int sage_attn_qk_int8_pv_f16(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v,
                             int v_dtype, const sage_tensor* o, int o_dtype,
                             const float* q_scale, const float* k_scale, const float* v_mean,
                             float* lse, int B, int Hq, int Hk, int M, int N, int D,
                             int is_causal, int qk_gran, int blkq, int warpq,
                             float sm_scale, int logit_mult_is_one, sage_stream_t stream);

/* ---- fused attention, INT8 QK^T + FP8 PV -------------------------------------------------------
 * Replaces qk_int8_sv_f8_accum_f32[_fuse_v_scale][_fuse_v_mean]_attn[_inst_buf] and
 * qk_int8_sv_f8_accum_f16_* (csrc/qattn/attn_cuda_sm89.h, qk_int_sv_f8_cuda_sm89.cuh:44-713) and the
 * fork's unfused qk_int8_sv_f8_accum_f32_attn (csrc/qattn/rocm/attn_rocm_gfx942.h:20-32).
 *   v_fp8: as produced by sage_quant_v_fp8 ([B,Hk,D,Npad], OCP e4m3fn);  v_scale fp32 [B,Hk,D]
 *   multiplied into the output columns (fuse_v_scale), v_mean optional. */
int sage_attn_qk_int8_pv_f8(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                            const sage_tensor* o, int o_dtype,
                            const float* q_scale, const float* k_scale, const float* v_scale,
                            const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N,
                            int D, int is_causal, int qk_gran, int blkq, int warpq,
                            float sm_scale, int logit_mult_is_one, sage_stream_t stream);

/* ---- fused attention with the Q quantizer folded into the kernel --------------------------------
 * Same operators as sage_attn_qk_int8_pv_{f16,f8}, but `q` is the fp16/bf16 query tensor: each wave
 * quantizes its own query rows in the kernel prologue with exactly the arithmetic of
 * sage_quant_qk_int8 (qk_gran per_warp -> SAGE_ROUND_CUDA, per_thread -> SAGE_ROUND_TRITON, blk 128),
 * which removes one launch and the int8 round trip of Q through HBM.  km (optional,
 * [B,Hk,D], dtype of q): when given, `lse` receives the FINAL natural-log LSE
 * lse2/log2(e) + (q.km)*sm_scale of core.py:651; otherwise lse2/log2(e).
 * Replaces the pair {quant_per_warp_int8_cuda | per_thread_int8 (Q half), qk_int8_sv_*_attn}. */
int sage_attn_fusedq_pv_f16(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v,
                            int v_dtype, const sage_tensor* o, int o_dtype, const float* k_scale,
                            const void* km, const float* v_mean, float* lse, int B, int Hq, int Hk,
                            int M, int N, int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                            sage_stream_t stream);
int sage_attn_fusedq_pv_f8(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                           const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                           const float* k_scale, const void* km, const float* v_scale,
                           const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                           int is_causal, int qk_gran, int warpq, float sm_scale, sage_stream_t stream);

/* ---- attention with an explicit attn_mask ----------------------------------------------------------
 * The attn_mask argument of sageattn_qk_int8_pv_fp16_triton (core.py:249-251,306-318; kernels
 * triton/attn_qk_int8_per_block.py:33-52, attn_qk_int8_per_thread.py:37-75).  Non-causal, 16-bit PV (v fp16 or
 * bf16, multiplied in its own type exactly as by sage_attn_qk_int8_pv_f16).
 * attn_mask: device pointer to a [B,Hq,M,N] VIEW given by mask_strides[4] in ELEMENTS (host array; 0 =
 * broadcast dimension).  mask_kind 1: bool/uint8, zero = masked (the reference adds -1e6 to the base-2
 * logit); 2: fp16, 3: bf16 additive mask, added to the base-2 logit exactly as the reference does (after
 * its sm_scale*log2(e) scaling).  Rows without any allowed key are undefined in the reference (they
 * depend on its 128x64 tile skipping) and here. */
int sage_attn_qk_int8_pv_f16_masked(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v,
                                    int v_dtype, const sage_tensor* o, int o_dtype,
                                    const float* q_scale, const float* k_scale, const void* attn_mask,
                                    int mask_kind, const int64_t* mask_strides, float* lse, int B, int Hq,
                                    int Hk, int M, int N, int D, int qk_gran, int blkq, int warpq,
                                    float sm_scale, int logit_mult_is_one, sage_stream_t stream);

/* ---- packed variable-length sequences (sageattn_varlen, core.py:363-477) ------------------------
 * q/k/v/o are packed [total_tokens, H, D] tensors described as sage_tensor with stride_b unused;
 * sequence s owns rows [cu_seqlens[s], cu_seqlens[s+1]) (int32, device memory, num_seqs+1 entries).
 * Quantization blocks restart at every sequence start (triton/quant_per_block_varlen.py:21-58); the
 * scale tensors are [num_seqs, H, G(max_seqlen)] (a private layout: the reference's cumulative block
 * offsets, quant_per_block_varlen.py:73-80, are not needed).  The mean vector is per (head, channel)
 * over ALL packed tokens, [1,H,D] (core.py:461).  FP16 PV only and no LSE, as in the reference.
 * Replace the Triton varlen quantizer + attn_qk_int8_block_varlen.py / attn_qk_int8_per_block_causal_varlen.py. */
int sage_quant_qk_int8_varlen(const sage_tensor* x, int dtype, const int* cu_seqlens, int num_seqs, int H,
                              int max_seqlen, int D, const void* mean, const sage_tensor* out, float* scale,
                              int gran, int is_key, int blk, int warp, float mult, int rounding,
                              sage_stream_t stream);
int sage_attn_qk_int8_pv_f16_varlen(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v,
                                    int v_dtype, const sage_tensor* o, int o_dtype,
                                    const float* q_scale, const float* k_scale,
                                    const int* cu_seqlens_q, const int* cu_seqlens_k, int num_seqs,
                                    int Hq, int Hk, int max_seqlen_q, int max_seqlen_k, int D,
                                    int is_causal, int qk_gran, int blkq, int warpq, float sm_scale,
                                    int logit_mult_is_one, sage_stream_t stream);

/* ---- ring attention merge (new; the reference only exposes return_lse, core.py:122-124) -------
 * In place: (o_acc, lse_acc) <- merge((o_acc, lse_acc), (o_blk, lse_blk)) with
 *   lse = logaddexp(lse_a, lse_b);  o = o_a*exp(lse_a-lse) + o_b*exp(lse_b-lse).
 * o_acc: fp32 [rows, D] contiguous; lse_acc / lse_blk: fp32 [rows] natural log;
 * o_blk: fp16/bf16 [rows, D] contiguous.
 * A side with lse = -inf is empty and weighs 0; an empty side's o may hold anything (an uninitialised accumulator with
 * lse_acc = -inf is the natural start of a ring, a fully masked block leaves its o undefined): NaN or Inf there never
 * reaches the result.  Both sides empty: (0, -inf). */
int sage_merge_attn_states(float* o_acc, float* lse_acc, const void* o_blk, int o_dtype,
                           const float* lse_blk, int64_t rows, int D, sage_stream_t stream);

/* Multi-way form: (o_out, lse_out) = merge of `count` block results (1 <= count <= SAGE_MERGE_MAX) in one pass,
 *   lse = log(sum_i exp(lse_i));  o = sum_i o_i * exp(lse_i - lse)   (blocks with lse_i = -inf weigh 0).
 * o_blks[i]: fp16/bf16 [rows, D] contiguous (o_dtype), lse_blks[i]: fp32 [rows] natural log; HOST arrays of
 * device pointers.  o_out: [rows, D] in o_dtype; lse_out: fp32 [rows] or NULL.  A ring step over P shards otherwise
 * passes the fp32 accumulator through HBM P times. */
#define SAGE_MERGE_MAX 16
int sage_merge_attn_states_multi(const void* const* o_blks, const float* const* lse_blks, int count,
                                 int o_dtype, void* o_out, float* lse_out, int64_t rows, int D,
                                 sage_stream_t stream);

/* lse_out[i] = lse2[i]/log2(e) + (corr ? corr[i]*sm_scale : 0)   (core.py:651), n elements. */
int sage_finish_lse(const float* lse2, const float* corr, float sm_scale, float* lse_out,
                    int64_t n, sage_stream_t stream);

/* ---- K smoothing + quantization in one call ------------------------------------------
 * = sage_k_mean + sage_quant_qk_int8(is_key = 1, mean = km, blk 64, mult 1), bit-identical, in TWO launches at every length:
 * the sequence is cut into at most 16 chunks whose column sums the quantizer finishes itself (one launch less than the pair).  gran: SAGE_GRAN_PER_BLOCK or SAGE_GRAN_PER_THREAD; km: [B,H,D] out (dtype of k); workspace as
 * sage_k_mean.  Replaces `k.mean` (core.py:612) + quant_per_block_int8_fuse_sub_mean_cuda (fused.cu:594-682) / the K half
 * of per_thread_int8 (triton/quant_per_thread.py:48-102,162-163). */
int sage_k_smooth_quant(const sage_tensor* k, int dtype, int B, int H, int N, int D, const sage_tensor* out,
                        float* scale, void* km, int gran, int rounding, void* workspace, sage_stream_t stream);

/* The whole K/V side of the FP8-PV operator's pre-pass as ONE call: km + INT8 K (as sage_k_smooth_quant) and the FP8 V^T
 * with its per-channel scale (as sage_quant_v_fp8 with v_mean = NULL, i.e. smooth_v = False), k and v of equal shape
 * [B,H,N,D].  At every length it runs as two launches (K and V column statistics per chunk; both quantizers, each finishing
 * its own statistics) instead of five.  Results are bit-identical to the two separate entry points.  Replaces core.py:612 + :621-624 (K half) + per_channel_fp8 (quant.py:225-322, fused.cu:262-427). */
size_t sage_kv_prepare_fp8_workspace_bytes(int B, int H, int N, int D);
int sage_kv_prepare_fp8(const sage_tensor* k, const sage_tensor* v, int dtype, int B, int H, int N, int D,
                        const sage_tensor* k_int8, float* k_scale, void* km, int gran, int rounding,
                        const sage_tensor* v_fp8, float* v_scale, float scale_max, void* workspace, sage_stream_t stream);

/* ---- one-call operators ---------------------------------------------------------------------------------------------
 * The whole body of sageattn_qk_int8_pv_fp16_cuda (core.py:604-651) / sageattn_qk_int8_pv_fp8_cuda (core.py:786-905)
 * below their argument checks as ONE call with ONE caller-provided workspace: km = mean(k) and the INT8 K quantizer,
 * the FP8 V^T quantizer (pv_f8), the Q quantizer (folded into the attention kernel's prologue unless fuse_q = 0),
 * the fused attention kernel and the LSE fix of core.py:651.  It sequences the library's own entry points on `stream`
 * (sage_k_smooth_quant | sage_kv_prepare_fp8, sage_quant_qk_int8, sage_attn_{fusedq,qk_int8}_pv_*, sage_finish_lse), so
 * results are bit-identical to calling those one by one.  q, k, v, o: fp16 or bf16 (one dtype), head_dim 64 or 128 (the
 * caller pads, core.py:592-601); lse: optional fp32 [B,Hq,M], receives the natural-log LSE of the un-smoothed logits.
 * opts: quantization granularity of the reference's `qk_quant_gran` (per_warp -> CUDA quantizer numerics, per_thread ->
 * Triton numerics, core.py:621-624); warpq 32 (16 = the reference's "fp16+fp32" per-warp variant, core.py:622); smooth_k
 * must be 1 (core.py:612; without smoothing use the separate entry points); fuse_q -1 = the library's choice; nwaves =
 * the per-call form of SAGE_TUNE_NWAVES (0 = the library's measured choice).
 * workspace: at least sage_sageattn_workspace_bytes(...) bytes, 16-byte aligned, private to the call until it has
 * finished on `stream`. */
typedef struct sage_op_opts {
  int qk_gran;  /* SAGE_GRAN_PER_WARP | SAGE_GRAN_PER_THREAD */
  int warpq;    /* 32 (or 16) */
  int smooth_k; /* 1 */
  int fuse_q;   /* -1 | 0 | 1 */
  int nwaves;   /* 0 | 4 | 8 */
  int reserved[3];
} sage_op_opts;
size_t sage_sageattn_workspace_bytes(int pv_fp8, int B, int Hq, int Hk, int M, int N, int D, int want_lse,
                                     const sage_op_opts* opts);
int sage_sageattn_pv_f16(const sage_tensor* q, const sage_tensor* k, const sage_tensor* v, int dtype,
                         const sage_tensor* o, float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal,
                         float sm_scale, const sage_op_opts* opts, void* workspace, size_t workspace_bytes,
                         sage_stream_t stream);
int sage_sageattn_pv_f8(const sage_tensor* q, const sage_tensor* k, const sage_tensor* v, int dtype,
                        const sage_tensor* o, float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal,
                        float sm_scale, float scale_max, const sage_op_opts* opts, void* workspace,
                        size_t workspace_bytes, sage_stream_t stream);

/* ==== sequence-parallel building blocks (new: the reference has no parallelism code; its hook is
 * return_lse, core.py:122-124, and its multi-GPU launcher delegates to xDiT, example/parallel_sageattn_cogvideo.py:40-52).
 * With ONE smoothing mean and ONE V scale for the whole sequence (statistics exchanged first: a few KB), the quantized
 * K/V shards of all ranks are exactly the operands of the unsharded operator, so a rank attends the gathered shards
 * with plain launches of the attention kernel: no per-shard LSE corrections, no per-shard outputs.
 * The exchange buffers are TILE-MAJOR: tile j (64 keys) of every (b, h_kv) is one contiguous block,
 *   k8 [tiles][B][Hk][64][D] int8, v fp16 [tiles][B][Hk][64][D] / v fp8 [tiles][B][Hk][D][64], k_scale [tiles][B][Hk][4|1],
 * so the tiles received from all ranks, stored one rank after the other, form one sequence for every head. ==== */

/* KV tile layout of an attention call: distance between consecutive 64-key tiles of one (b, h_kv).
 * k_tile_stride: int8 elements (= bytes) in k8; v_tile_stride: elements of v (fp16: 2 bytes each; fp8: bytes);
 * 0 = dense (64 * stride_n; fp8: 64).  Within a tile rows keep the sage_tensor's stride_n.
 * ks_stride_{b,h,tile}: floats between the k scales of consecutive batches / kv heads / 64-key tiles; all 0 = the dense
 * [B,Hk,Gk] layout.  per_thread scales are read 16 B at a time: multiples of 4. */
typedef struct sage_kv_layout {
  int64_t k_tile_stride, v_tile_stride;
  int64_t ks_stride_b, ks_stride_h, ks_stride_tile;
} sage_kv_layout;

/* sage_attn_qk_int8_pv_{f16,f8} on K/V operands in an explicit tile layout (non-causal or causal; no v_mean).
 * The raw base-2 LSE is returned as there. */
int sage_attn_qk_int8_pv_f16_kvtiles(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                     const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                     const sage_kv_layout* kv_layout, float* lse, int B, int Hq, int Hk, int M, int N,
                                     int D, int is_causal, int qk_gran, int blkq, int warpq, float sm_scale,
                                     sage_stream_t stream);
int sage_attn_qk_int8_pv_f8_kvtiles(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                    const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                    const float* v_scale, const sage_kv_layout* kv_layout, float* lse, int B, int Hq,
                                    int Hk, int M, int N, int D, int is_causal, int qk_gran, int blkq, int warpq,
                                    float sm_scale, sage_stream_t stream);

/* Per-channel statistics of a [B,H,N,D] fp16/bf16 tensor over its N rows: stats fp32 [B,H,3,D] = (max, min, sum),
 * deterministic two-level reduction.  For N % 16 != 0 the rows [N, ceil16(N)) count as zeros (the reference's padded
 * amax, fused.cu:335): max = max(true max, 0), min = min(true min, 0); max|x| and the sum are those of the N rows.  The local halves of `k.mean` (core.py:612) and of the per-channel amax of
 * per_channel_fp8 (quant.py:225-322, fused.cu:316-427).  workspace: sage_seq_stats_workspace_bytes bytes. */
size_t sage_seq_stats_workspace_bytes(int B, int H, int N, int D);
int sage_seq_stats(const sage_tensor* x, int dtype, int B, int H, int N, int D, float* stats, void* workspace,
                   sage_stream_t stream);

/* Combine the statistics of `parts` sequence shards (k_stats / v_stats: fp32 [BH][3][D] per shard, shard p at
 * + p*part_stride floats, e.g. an all-gather of sage_seq_stats results; v_stats may be NULL) into the operands of the
 * quantizers:
 *   km [BH][D] (dtype) = sum of sums / n_total                      (core.py:612 over the WHOLE sequence)
 *   v_scale fp32 [BH][D] = max |v| / scale_max,  v_coef fp32 [BH][2][D] = (0, scale_max / max |v|)   (quant.py:228,318-321)
 *   (max |v| == 0: v_scale = 0 and the coefficient 0, see sage_quant_v_fp8)
 * Fixed summation order: every rank computes identical bits from the same gathered statistics. */
int sage_kv_stats_reduce(const float* k_stats, const float* v_stats, int parts, int64_t part_stride, int BH, int D,
                         int64_t n_total, int dtype, float scale_max, void* km, float* v_scale, float* v_coef,
                         sage_stream_t stream);

/* sage_quant_qk_int8 for K with tile-major results: out row r of (b,h) is written at
 * out->data + b*stride_b + h*stride_h + (r/64)*out_tile_stride + (r%64)*stride_n, its scales at
 * scale + b*scale_strides[0] + h*scale_strides[1] + (r/64)*scale_strides[2] (+ 0..3).  blk = 64. */
int sage_quant_k_int8_kvtiles(const sage_tensor* k, int dtype, int B, int H, int N, int D, const void* mean,
                              const sage_tensor* out, int64_t out_tile_stride, float* scale,
                              const int64_t* scale_strides, int gran, int rounding, sage_stream_t stream);

/* Second half of sage_quant_v_fp8 alone: v -> e4m3 with GIVEN coefficients v_coef [B,H,2,D] = (mean, scale_max/amax)
 * (sage_kv_stats_reduce), token block t of (b,h) written at v_fp8->data + b*stride_b + h*stride_h + t*out_tile_stride
 * (bytes; 0 = 64: the dense [B,H,D,Npad] layout), channel d at + d*stride_n. */
int sage_quant_v_fp8_apply(const sage_tensor* v, int dtype, int B, int H, int N, int D, const sage_tensor* v_fp8,
                           int64_t out_tile_stride, const float* v_coef, sage_stream_t stream);

/* sage_merge_attn_states_multi for partial results that share one smoothing vector: the inputs' LSE are multiplied by
 * lse_in_mult first (1/log2(e) for the raw base-2 LSE of the attention entry points) and
 * lse_out = log(sum) + (corr ? corr*corr_mult : 0)   (core.py:651 applied once, after the merge). */
int sage_merge_attn_states_multi_ex(const void* const* o_blks, const float* const* lse_blks, int count, int o_dtype,
                                    void* o_out, float* lse_out, int64_t rows, int D, float lse_in_mult,
                                    const float* corr, float corr_mult, sage_stream_t stream);

/* ==== block-sparse attention (new: SpargeAttn-style block maps, sliding-tile / window patterns, text and padding
 * cut-outs.  The reference has no counterpart beyond the tile skipping of its masked Triton kernels,
 * triton/attn_qk_int8_per_block.py:38-39; geometry: those kernels' 128x64 tile) ====
 * block_map[b, h_q, i, j] != 0: query rows [128 i, 128 i + 128) of head h_q attend keys [64 j, 64 j + 64).  Tiles that are
 * off are neither copied nor computed; inside an active tile only the sequence end (N % 64) masks keys.  Non-causal.
 * Query rows of a block row without any active tile are DEFINED: o = 0, lse = -inf (sage_attn_qk_int8_pv_f16_masked
 * leaves such rows undefined).
 *
 * The attention kernels take the map as compacted tile lists, a caller-owned buffer of
 * sage_block_sparse_workspace_bytes(B,Hq,M,N) bytes (0 for non-positive sizes), 16-byte aligned: one row of int32 per
 * (b, h_q, block row) = [count, the active tile indices ascending, then the last of them repeated (>= 5 times)]; a row has
 * 1 + ceil(N/64) + 5 entries rounded up to a multiple of 4.  A static pattern is compacted once and the lists are reused.
 * sage_block_map_compact: block_map is a device pointer to a uint8/bool [B,Hq,ceil(M/128),ceil(N/64)] VIEW given by
 * map_strides[4] in ELEMENTS (host array; 0 = broadcast dimension, as the attn_mask of sage_attn_qk_int8_pv_f16_masked).
 * One wave per list row (ballot + prefix count): deterministic, no atomics. */
size_t sage_block_sparse_workspace_bytes(int B, int Hq, int M, int N);
int sage_block_map_compact(const void* block_map, const int64_t* map_strides, int B, int Hq, int M, int N,
                           int32_t* block_lists, int64_t block_lists_bytes, sage_stream_t stream);

/* sage_attn_qk_int8_pv_{f16,f8} and sage_attn_fusedq_pv_{f16,f8} over the active tiles of a block map: the arguments of the
 * dense twin, then the lists (block_lists, block_lists_bytes >= sage_block_sparse_workspace_bytes).  Same loop and same
 * arithmetic in the same order as the dense kernel run on the active tiles gathered into one contiguous K/V: results are
 * bit-identical to that.  Replace sage_attn_qk_int8_pv_f16_masked on an expanded [B,H,M,N] mask for block-granular
 * patterns, and extend it to FP8 PV and the fused Q quantizer.  Workgroups always have 4 waves (128 rows = one block row of
 * the map): SAGE_TUNE_NWAVES does not apply.  Not combinable: is_causal != 0 and v_mean != NULL return
 * SAGE_ERR_UNSUPPORTED; there is no varlen, attn_mask or kv_layout form.  The kernels trust the lists (counts, ascending
 * indices < ceil(N/64), the padded tail): pass what sage_block_map_compact wrote for the same (B, Hq, M, N).  The rows of
 * empty block rows are written by a second, tiny launch on the same stream. */
int sage_attn_qk_int8_pv_f16_blocksparse(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v,
                                         int v_dtype, const sage_tensor* o, int o_dtype,
                                         const float* q_scale, const float* k_scale, const float* v_mean,
                                         float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                         int is_causal, int qk_gran, int blkq, int warpq,
                                         float sm_scale, int logit_mult_is_one, const int32_t* block_lists,
                                         int64_t block_lists_bytes, sage_stream_t stream);
int sage_attn_qk_int8_pv_f8_blocksparse(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                        const sage_tensor* o, int o_dtype,
                                        const float* q_scale, const float* k_scale, const float* v_scale,
                                        const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N,
                                        int D, int is_causal, int qk_gran, int blkq, int warpq,
                                        float sm_scale, int logit_mult_is_one, const int32_t* block_lists,
                                        int64_t block_lists_bytes, sage_stream_t stream);
int sage_attn_fusedq_pv_f16_blocksparse(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v,
                                        int v_dtype, const sage_tensor* o, int o_dtype, const float* k_scale,
                                        const void* km, const float* v_mean, float* lse, int B, int Hq, int Hk,
                                        int M, int N, int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                                        const int32_t* block_lists, int64_t block_lists_bytes, sage_stream_t stream);
int sage_attn_fusedq_pv_f8_blocksparse(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                       const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                       const float* k_scale, const void* km, const float* v_scale,
                                       const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                       int is_causal, int qk_gran, int warpq, float sm_scale,
                                       const int32_t* block_lists, int64_t block_lists_bytes, sage_stream_t stream);

/* ... with SpargeAttn's second stage, the P.V skip (pvthreshd): inside the tile loop a wave -- 32 query rows of a 128-row
 * q-block -- leaves out the exponentials, the packing of P, the row sums and the P.V products of a tile whose scores are
 * all negligible against what its rows have already seen.  The arguments of the _blocksparse twin, then
 *   pv_thresh  device, fp32 [Hq], 4-byte aligned, required: the threshold of every query head, a positive number in the
 *              natural-log units of the scaled logits (the units of lse; the kernel multiplies it by log2 e)
 *   skipped    device, int32 [B, Hq, ceil(M/128), 4], 4-byte aligned, or NULL: per wave the number of tiles it skipped
 * The rule, for a wave and the tile at list position pos of its q-block's list:
 *   m_ref[r]  the kernel's running reference maximum of row r when the tile is reached (after the lazy rescale for this
 *             tile).  It lags the true running maximum of the row by at most lazy = 6 ln 2 (FP16 / BF16 PV), 3 ln 2 (FP8 PV).
 *   t[r]      the row maximum of this tile's logits, over keys < N only.
 *   The wave skips the tile iff pos > 0 and, for every row r of the wave with r < M, t[r] <= m_ref[r] - pv_thresh[h].
 * Rows at or beyond M take no part (the padded rows of a ragged q-block would otherwise veto every skip).  A skipped tile
 * changes nothing for the wave: running maximum, row sums and O stay as they are, as if the tile were not in the wave's
 * list -- o and lse of the wave's rows are bit-identical to the _blocksparse twin run without that tile.  So every P of a
 * skipped tile is at most e^-pv_thresh relative to the row's true running maximum, a tile whose gap is at least
 * pv_thresh + lazy on all valid rows is certainly skipped, and the first tile of a list never is.  A threshold that is not
 * greater than 0, +inf or NaN means "never skip" for that head (mapped to +inf by the kernel; the tensor is not read on
 * the host).  Every entry of skipped is written by every call: waves whose rows are all >= M and the waves of empty
 * q-blocks report 0.  No atomics.  A skipping wave issues the same tile copies, waits and barriers as a computing one; it
 * saves the V fragment reads, the softmax vector work and the P.V MFMAs.
 * Checked before any launch: pv_thresh NULL or unaligned, skipped unaligned -> SAGE_ERR_INVALID_ARGUMENT; is_causal != 0
 * and v_mean != NULL -> SAGE_ERR_UNSUPPORTED, as for the twins. */
int sage_attn_qk_int8_pv_f16_blocksparse_pvskip(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v,
                                                int v_dtype, const sage_tensor* o, int o_dtype, const float* q_scale,
                                                const float* k_scale, const float* v_mean, float* lse, int B, int Hq,
                                                int Hk, int M, int N, int D, int is_causal, int qk_gran, int blkq,
                                                int warpq, float sm_scale, int logit_mult_is_one,
                                                const int32_t* block_lists, int64_t block_lists_bytes,
                                                const float* pv_thresh, int32_t* skipped, sage_stream_t stream);
int sage_attn_qk_int8_pv_f8_blocksparse_pvskip(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                               const sage_tensor* o, int o_dtype, const float* q_scale,
                                               const float* k_scale, const float* v_scale, const float* v_mean,
                                               float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal,
                                               int qk_gran, int blkq, int warpq, float sm_scale, int logit_mult_is_one,
                                               const int32_t* block_lists, int64_t block_lists_bytes,
                                               const float* pv_thresh, int32_t* skipped, sage_stream_t stream);
int sage_attn_fusedq_pv_f16_blocksparse_pvskip(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                               const sage_tensor* v, int v_dtype, const sage_tensor* o, int o_dtype,
                                               const float* k_scale, const void* km, const float* v_mean, float* lse,
                                               int B, int Hq, int Hk, int M, int N, int D, int is_causal, int qk_gran,
                                               int warpq, float sm_scale, const int32_t* block_lists,
                                               int64_t block_lists_bytes, const float* pv_thresh, int32_t* skipped,
                                               sage_stream_t stream);
int sage_attn_fusedq_pv_f8_blocksparse_pvskip(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                              const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                              const float* k_scale, const void* km, const float* v_scale,
                                              const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N,
                                              int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                                              const int32_t* block_lists, int64_t block_lists_bytes,
                                              const float* pv_thresh, int32_t* skipped, sage_stream_t stream);

/* ==== per-batch key lengths on the dense padded layout (new: batches whose rows have different numbers of valid keys --
 * cross-attention over padded prompts, joint video + text attention, batched prompt sets.  The reference's routes are an
 * attn_mask, core.py:249-251, or repacking for sageattn_varlen, core.py:363-477) ====
 * kv_lens: device, int32 [B], 4-byte aligned.  len_b = clamp(kv_lens[b], 0, N).  The rule:
 *   - For every b with len_b > 0 the rows of batch b in o (and lse) are BIT-IDENTICAL to the twin without kv_lens called on
 *     the slices q[b:b+1], k[b:b+1, :, :len_b], v[b:b+1, :, :len_b] with every other argument equal.  For the attention entry
 *     points "k" and "v" are their quantized operands; the pre-pass twins below produce exactly those: km[b], the INT8 rows
 *     < len_b with their scales, v_scale[b] and the V^T columns < len_b equal the results of the twin on the slice.
 *   - Nothing in rows >= len_b of K or V influences any output: not their values, NaN and Inf included.  The pre-pass takes
 *     every statistic (smoothing mean, block and per-thread scales, per-channel max|v|) over the rows < len_b only and never
 *     loads the others; the attention kernels end their K / V buffer descriptors with row len_b - 1.
 *   - is_causal is top-left aligned, as in the dense operator: query row i sees keys 0 .. min(i, len_b - 1).
 *   - len_b == 0: o = 0, lse = -inf (the block-sparse convention), written by a second, tiny launch; the smoothing mean of
 *     that batch is 0, not 0/0, so that the LSE correction of the fused-Q forms stays -inf.  Its scales and v_scale are
 *     unspecified and never read.
 *   - The lengths are read on the device only: no host synchronisation; a call captures into a HIP graph, and a replay
 *     reads the lengths the buffer holds then.
 * Grids, scale arrays ([B,H,ceil(N/64)(*4)]), the V^T row length (64*ceil(N/64)) and the workgroup geometry are those of N;
 * the bits do not depend on the geometry.  Scales of blocks wholly beyond len_b, INT8 rows >= len_b and V^T columns
 * >= 64*ceil(len_b/64) are unspecified and never read.
 * Not built, SAGE_ERR_UNSUPPORTED from the argument check: kv_lens of these DENSE entry points together with a block map, an
 * attn_mask, cu_seqlens or a kv_layout (the entry points below have none of those arguments; a block map with lengths has
 * entry points of its own, sage_attn_*_blocksparse_kvlen further down).  kv_lens NULL or misaligned:
 * SAGE_ERR_INVALID_ARGUMENT.  All checks run before any launch. */

/* sage_k_smooth_quant with kv_lens: the mean of batch b is the sum over its rows < len_b, chunked as a call on len_b rows
 * chunks them and added in the same order, divided by len_b.  The K quantizer treats rows >= len_b as absent for the block
 * and per-thread scales.  km: 16-byte aligned.  workspace as sage_k_smooth_quant (for N rows).  Two launches. */
int sage_k_smooth_quant_kvlen(const sage_tensor* k, int dtype, int B, int H, int N, int D, const sage_tensor* out,
                              float* scale, void* km, int gran, int rounding, void* workspace, const int32_t* kv_lens,
                              sage_stream_t stream);
/* sage_kv_prepare_fp8 with kv_lens: the K half as above; the per-channel max|v| of batch b over its rows < len_b only; the V^T
 * image gets zero bytes in columns [len_b, 64*ceil(len_b/64)) (the attention kernel's descriptor covers the whole last tile,
 * and an e4m3 NaN byte times P = 0 is NaN).  workspace as sage_kv_prepare_fp8 (for N rows).  Two launches. */
int sage_kv_prepare_fp8_kvlen(const sage_tensor* k, const sage_tensor* v, int dtype, int B, int H, int N, int D,
                              const sage_tensor* k_int8, float* k_scale, void* km, int gran, int rounding,
                              const sage_tensor* v_fp8, float* v_scale, float scale_max, void* workspace,
                              const int32_t* kv_lens, sage_stream_t stream);

/* sage_attn_qk_int8_pv_{f16,f8} and sage_attn_fusedq_pv_{f16,f8} with kv_lens: the arguments of the twin, then kv_lens.  The
 * same pipelined loop, per-thread and per-warp scales, the fused Q quantizer, FP16 / BF16 / FP8 PV, LSE, GQA, both head dims
 * and both workgroup geometries (SAGE_TUNE_NWAVES applies). */
int sage_attn_qk_int8_pv_f16_kvlen(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v, int v_dtype,
                                   const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                   const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                   int is_causal, int qk_gran, int blkq, int warpq, float sm_scale, int logit_mult_is_one,
                                   const int32_t* kv_lens, sage_stream_t stream);
int sage_attn_qk_int8_pv_f8_kvlen(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                  const sage_tensor* o, int o_dtype, const float* q_scale, const float* k_scale,
                                  const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                  int N, int D, int is_causal, int qk_gran, int blkq, int warpq, float sm_scale,
                                  int logit_mult_is_one, const int32_t* kv_lens, sage_stream_t stream);
int sage_attn_fusedq_pv_f16_kvlen(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v,
                                  int v_dtype, const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                  const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                  int is_causal, int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens,
                                  sage_stream_t stream);
int sage_attn_fusedq_pv_f8_kvlen(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_fp8,
                                 const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                 const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                 int N, int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                                 const int32_t* kv_lens, sage_stream_t stream);

/* ==== per-batch key lengths for block-sparse attention (joint video + text attention over a guidance batch whose prompts
 * differ in length: a padded batch with kv_lens that wants the block-sparse kernels) ====
 * A block map cuts at 64-key tiles; a prompt ends where it ends.  kv_lens, len_b as above; ntk_b = ceil(len_b / 64).  The rule:
 *   - For every b with len_b > 0 the rows of batch b in o, lse and the skip counters are BIT-IDENTICAL to the
 *     _blocksparse twin (with pv_thresh: the _blocksparse_pvskip twin) called on the slices q[b:b+1], k[b:b+1, :, :len_b],
 *     v[b:b+1, :, :len_b] with the lists of the caller's map cut to its first ntk_b key-tile columns.
 *   - Tiles j >= ntk_b of a list are treated as off; tile ntk_b - 1 is masked at len_b, not at N.
 *   - A q-block whose list has no entry < ntk_b has o = 0, lse = -inf and counters 0 -- the convention of empty q-blocks.
 *     With len_b == 0 every row of the batch has these values.
 *   - Nothing in rows >= len_b of K or V influences any output, NaN and Inf included ("K" and "V" are the quantized operands:
 *     make them with sage_k_smooth_quant_kvlen / sage_kv_prepare_fp8_kvlen, whose statistics run over the rows < len_b).
 *   - The lists are read-only: the kernel counts the entries < ntk_b of a row (the list ascends) and walks that prefix.  Lists
 *     compacted once for (B, Hq, M, N) stay valid for any kv_lens, call after call.
 *   - The lengths are read on the device only; a call captures into a HIP graph and a replay reads the lengths held then.
 * The arguments of the _blocksparse_pvskip twin, then kv_lens.  pv_thresh == NULL selects the kernel without the P.V skip
 * (skipped is then not read); otherwise pv_thresh and skipped as for the twin.  kv_lens NULL or misaligned:
 * SAGE_ERR_INVALID_ARGUMENT; every other status as the twin gives it.  All checks run before any launch.  The rows of the
 * emptied q-blocks are written by a second, tiny launch on the same stream.
 * Not built: query lengths, a causal form, and kv_lens on the one-call operators.  (The calibration entry points have twins
 * with kv_lens: sage_attn_tile_mass_kvlen and sage_block_plan_recall_kvlen, at the end of this file.) */
int sage_attn_qk_int8_pv_f16_blocksparse_kvlen(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v,
                                               int v_dtype, const sage_tensor* o, int o_dtype, const float* q_scale,
                                               const float* k_scale, const float* v_mean, float* lse, int B, int Hq,
                                               int Hk, int M, int N, int D, int is_causal, int qk_gran, int blkq,
                                               int warpq, float sm_scale, int logit_mult_is_one,
                                               const int32_t* block_lists, int64_t block_lists_bytes,
                                               const float* pv_thresh, int32_t* skipped, const int32_t* kv_lens,
                                               sage_stream_t stream);
int sage_attn_qk_int8_pv_f8_blocksparse_kvlen(const sage_tensor* q8, const sage_tensor* k8, const sage_tensor* v_fp8,
                                              const sage_tensor* o, int o_dtype, const float* q_scale,
                                              const float* k_scale, const float* v_scale, const float* v_mean,
                                              float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal,
                                              int qk_gran, int blkq, int warpq, float sm_scale, int logit_mult_is_one,
                                              const int32_t* block_lists, int64_t block_lists_bytes,
                                              const float* pv_thresh, int32_t* skipped, const int32_t* kv_lens,
                                              sage_stream_t stream);
int sage_attn_fusedq_pv_f16_blocksparse_kvlen(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                              const sage_tensor* v, int v_dtype, const sage_tensor* o, int o_dtype,
                                              const float* k_scale, const void* km, const float* v_mean, float* lse,
                                              int B, int Hq, int Hk, int M, int N, int D, int is_causal, int qk_gran,
                                              int warpq, float sm_scale, const int32_t* block_lists,
                                              int64_t block_lists_bytes, const float* pv_thresh, int32_t* skipped,
                                              const int32_t* kv_lens, sage_stream_t stream);
int sage_attn_fusedq_pv_f8_blocksparse_kvlen(const sage_tensor* q, int q_dtype, const sage_tensor* k8,
                                             const sage_tensor* v_fp8, const sage_tensor* o, int o_dtype,
                                             const float* k_scale, const void* km, const float* v_scale,
                                             const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N,
                                             int D, int is_causal, int qk_gran, int warpq, float sm_scale,
                                             const int32_t* block_lists, int64_t block_lists_bytes,
                                             const float* pv_thresh, int32_t* skipped, const int32_t* kv_lens,
                                             sage_stream_t stream);

/* ==== block-map predictor (new: makes the tile lists above from Q and K at run time, after SpargeAttn's first stage --
 * pooled scores gated by the self-similarity of the blocks.  The reference has no counterpart; the rule below is this
 * library's own statement).  Non-causal.  All arithmetic is fp32; inputs are finite. ====
 *
 * Block statistics of x [B,H,N,D] fp16/bf16 for blocks of blk rows (the last one may be ragged; c = its row count), with
 * x'_r = float(x_r) - float(mean) (mean: optional [B,H,D], dtype of x, contiguous, 16-byte aligned):
 *   pooled[b,h,i,:] = (sum_r x'_r) / c                      fp32 [B,H,ceil(N/blk),D] contiguous, 16-byte aligned
 *   sim[b,h,i]      = |sum_r x'_r / |x'_r| |^2 / c^2        fp32 [B,H,ceil(N/blk)]   contiguous
 * sim is the mean of the c x c matrix of cosines between the rows of the block (1 = all rows parallel), taken without
 * forming the matrix; a row of zero norm contributes the zero vector.  blk in {64,128}; D in {64,128}; x as the k of
 * sage_k_mean.  One pass over x, deterministic (fixed summation order, no atomics).  Q is pooled with blk = 128 and no mean,
 * K with blk = 64 and mean = the smoothing mean km of the K quantizer: without it every K block looks self-similar, because
 * all rows share the mean. */
int sage_block_pool_sim(const sage_tensor* x, int dtype, int B, int H, int N, int D, int blk, const void* mean,
                        float* pooled, float* sim, sage_stream_t stream);

/* Selection, per query head h_q (kv head h_k = h_q / (Hq/Hk)) and q-block i, from the statistics of Q (blk 128, M rows) and K
 * (blk 64, N rows), with the per-head thresholds simthreshd1[h_q] and cdfthreshd[h_q] (fp32 [Hq], device memory):
 *   key block j is ELIGIBLE if sim_k[b,h_k,j] > simthreshd1, q-block i SELF-SIMILAR if sim_q[b,h_q,i] > simthreshd1;
 *   p = softmax over the eligible j of sm_scale * dot(pooled_q[b,h_q,i], pooled_k[b,h_k,j]);
 *   SELECTED = the shortest prefix of the eligible j in descending p (ties: the lower j first) whose sum is
 *   >= cdfthreshd * sum(p); never empty when an eligible block exists; cdfthreshd >= 1 selects every eligible block;
 *   tile (i, j) is ON if j is selected, or j is not eligible, or i is not self-similar (blocks whose rows disagree cannot be
 *   summarised by their mean, so they are always computed).  Every q-block keeps at least one tile.
 * block_lists receives exactly what sage_block_map_compact writes for that map (same sizes and alignment:
 * sage_block_sparse_workspace_bytes(B,Hq,M,N)); block_map (optional) receives the map itself, uint8 [B,Hq,ceil(M/128),
 * ceil(N/64)] contiguous.  One wave per list row; deterministic, no atomics.  The row of p is kept in LDS: at most
 * SAGE_SPARGE_MAX_KEY_TILES key blocks (N <= 131072), SAGE_ERR_TOO_LARGE beyond.  sm_scale positive and finite. */
#define SAGE_SPARGE_MAX_KEY_TILES 2048
int sage_block_select_cdf(const float* pooled_q, const float* sim_q, const float* pooled_k, const float* sim_k,
                          int B, int Hq, int Hk, int M, int N, int D, float sm_scale, const float* simthreshd1,
                          const float* cdfthreshd, int32_t* block_lists, int64_t block_lists_bytes,
                          uint8_t* block_map, sage_stream_t stream);

/* Selection with a choice of rule and with key blocks pinned on (text tokens at one end of the key sequence, an
 * attention-sink block).  Statistics, ELIGIBLE and SELF-SIMILAR as for sage_block_select_cdf; ntk = ceil(N/64):
 *   key block j is KEPT if j < keep_first or j >= ntk - keep_last (ints >= 0, one pair per call; values beyond ntk act as ntk);
 *   j is a CANDIDATE if it is eligible and not kept; n = the number of candidates of (b, h_q) (it depends on h_q through
 *   simthreshd1[h_q]);  s_j = sm_scale * dot(pooled_q[b,h_q,i], pooled_k[b,h_k,j]) in fp32.
 *   rule SAGE_SELECT_CDF   rule_param = cdfthreshd[h_q]: the rule of sage_block_select_cdf with "eligible" read as
 *                          "candidate" -- the softmax of s and its mass run over the candidates only.  With keep_first =
 *                          keep_last = 0 it IS that rule: sage_block_select_cdf is this call, bit for bit.
 *   rule SAGE_SELECT_TOPK  rule_param = topk[h_q], the fraction of the candidates each q-block may attend:
 *                          kcount = n if !(topk < 1) (1 and above, and NaN), otherwise
 *                          kcount = min(n, max(1, (int)ceilf(topk * (float)n))), the product ONE fp32 multiplication;
 *                          SELECTED = the kcount candidates with the greatest s (equal values: the lower j first; +0 and -0
 *                          are equal).  No exponential is taken.
 *   tile (i, j) is ON if j is selected, or j is not a candidate, or i is not self-similar.  If n == 0 every tile of the row
 *   is on.  Every q-block keeps at least one tile.
 * Consequence of TOPK: every self-similar q-block of one (b, h_q) has exactly (ntk - n) + kcount active tiles -- lists of
 * equal length per head, a cost known before the call runs.
 * rule_param is fp32 [Hq] in device memory.  Outputs, limits and argument checks as for sage_block_select_cdf; an unknown
 * rule, a NULL rule_param and a negative keep_first / keep_last return SAGE_ERR_INVALID_ARGUMENT.  TOPK needs no softmax
 * and no float sums: scores become order-preserving unsigned keys and the kernel bisects on the key by counting. */
#define SAGE_SELECT_CDF  0
#define SAGE_SELECT_TOPK 1
int sage_block_select(const float* pooled_q, const float* sim_q, const float* pooled_k, const float* sim_k,
                      int B, int Hq, int Hk, int M, int N, int D, float sm_scale, const float* simthreshd1,
                      int rule, const float* rule_param /* cdfthreshd or topk, fp32 [Hq] */,
                      int keep_first, int keep_last, int32_t* block_lists, int64_t block_lists_bytes,
                      uint8_t* block_map, sage_stream_t stream);

/* The predictor with per-batch key lengths (kv_lens, len_b, ntk_b as for sage_attn_*_blocksparse_kvlen): the twins'
 * arguments, then kv_lens (NULL or misaligned: SAGE_ERR_INVALID_ARGUMENT; every other status as the twin).  Grids, strides
 * and output layouts are those of N.
 * sage_block_pool_sim_kvlen pools block i of batch b over its c = min(blk, len_b - blk*i) valid rows; rows >= len_b are
 * never loaded.  The statistics of the blocks of batch b below ceil(len_b / blk) are bit-identical to those of the twin on
 * x[b:b+1, :, :len_b]; those of blocks wholly beyond the length are unspecified and never read.  (Pool K with it; Q has no
 * lengths and goes through sage_block_pool_sim.)
 * sage_block_select_kvlen applies the rule of sage_block_select with ntk_b in the place of ntk everywhere: KEPT is
 * j < keep_first or j >= ntk_b - keep_last (keep_last pins the last VALID blocks), CANDIDATE, n and kcount follow, and key
 * blocks j >= ntk_b do not exist -- their tiles are off and their map columns are written 0.  With len_b == 0 every list of
 * the batch has count 0: the one exception to "every q-block keeps at least one tile".  For len_b > 0 the count and the
 * entries of every list row of batch b equal those sage_block_select writes for the slice (statistics of the slice, N =
 * len_b); the row stride of the lists and of the map stays that of N. */
int sage_block_pool_sim_kvlen(const sage_tensor* x, int dtype, int B, int H, int N, int D, int blk, const void* mean,
                              float* pooled, float* sim, const int32_t* kv_lens, sage_stream_t stream);
int sage_block_select_kvlen(const float* pooled_q, const float* sim_q, const float* pooled_k, const float* sim_k,
                            int B, int Hq, int Hk, int M, int N, int D, float sm_scale, const float* simthreshd1,
                            int rule, const float* rule_param, int keep_first, int keep_last, int32_t* block_lists,
                            int64_t block_lists_bytes, uint8_t* block_map, const int32_t* kv_lens, sage_stream_t stream);

/* ==== calibration of the predictor (new: what a block map loses, measured on the operands of the attention kernels; the
 * instrument behind a threshold search such as SpargeAttn's tuning mode.  The reference has no counterpart.) ====
 *
 * Exact tile mass.  For b, query head h, q-block i (rows [128 i, 128 i + 128), of which c_i = min(128, M - 128 i) are valid)
 * and key tile j (keys [64 j, 64 j + 64), only keys < N):
 *   mass[b,h,i,j] = (1 / c_i) * sum over the valid rows r of the q-block, sum over the keys n of the tile, of P[r, n]
 * where P[r, :] is the softmax over ALL keys < N of the logits the attention kernels exponentiate,
 *   S[r,n] * q_scale(r) * k_scale(n) * logit_mult,   S = q8 . k8 in int32,
 * logit_mult as logit_mult_is_one / sm_scale of sage_attn_qk_int8_pv_f16 select it, the scales indexed as that call indexes
 * them for SAGE_GRAN_PER_WARP and SAGE_GRAN_PER_THREAD (blkk = warpk = 64).  Non-causal, no mask.  mass is fp32
 * [B,Hq,ceil(M/128),ceil(N/64)] contiguous, 4-byte aligned; every entry is written by every call, each mass[b,h,i,:] sums
 * to 1 up to rounding, and rows >= M contribute nothing.  Deterministic: no atomics, two calls give the same bits.
 * q8, k8, q_scale, k_scale, B .. logit_mult_is_one: as for sage_attn_qk_int8_pv_f16 (D in {64,128}, Hq a multiple of Hk, any
 * M, N >= 1, any strides that call takes).  Checked before the launch: a null or misaligned pointer (k_scale: 16 bytes for
 * SAGE_GRAN_PER_THREAD) and inconsistent sizes SAGE_ERR_INVALID_ARGUMENT, another head_dim SAGE_ERR_UNSUPPORTED_HEAD_DIM,
 * SAGE_GRAN_PER_BLOCK SAGE_ERR_UNSUPPORTED (the block-sparse operators do not take it either).  Q and K are addressed with
 * 64-bit offsets, so there is no 2 GiB slice window and no SAGE_ERR_TOO_LARGE short of 2^31 q-blocks.
 * Two passes over the key tiles (row maximum and row sum; then the probabilities), QK^T only: twice the MFMA work of
 * the dense call's QK^T, two exponentials per score, no P.V. */
int sage_attn_tile_mass(const sage_tensor* q8, const sage_tensor* k8, const float* q_scale, const float* k_scale,
                        int B, int Hq, int Hk, int M, int N, int D, int qk_gran, int blkq, int warpq,
                        float sm_scale, int logit_mult_is_one, float* mass, sage_stream_t stream);

/* Recall of a plan: per list row (b, h_q, q-block i) of block_lists (as sage_block_map_compact / sage_block_select write them
 * for the same B, Hq, M, N)
 *   recall[b,h,i] = sum of mass[b,h,i,j] over the listed tiles j,   kept[b,h,i] = the row's count;
 * an empty row gives 0 and 0.  recall fp32 and kept int32 [B,Hq,ceil(M/128)] contiguous, 4-byte aligned.  One wave per list
 * row; the sum runs in tile slots (lane j % 64 adds its listed tiles in ascending order, then one fixed tree over the lanes),
 * so it is deterministic and a list that keeps a superset of tiles never gets a smaller recall, in fp32 too (mass >= 0).
 * The lists are trusted as by the attention kernels.  Argument checks as sage_block_map_compact. */
int sage_block_plan_recall(const int32_t* block_lists, int64_t block_lists_bytes, const float* mass, int B, int Hq, int M,
                           int N, float* recall, int32_t* kept, sage_stream_t stream);

/* Calibration with per-batch key lengths (kv_lens, len_b = clamp(kv_lens[b], 0, N), ntk_b = ceil(len_b / 64) as for
 * sage_attn_*_blocksparse_kvlen): the calibration sees the operands, the key range and the lists of the attention call it
 * calibrates.  Each entry point takes the arguments of its twin, then kv_lens (NULL or misaligned:
 * SAGE_ERR_INVALID_ARGUMENT; every other status as the twin gives it); all checks run before the launch.  Grids, strides and
 * output layouts are those of N.  The lengths are read on the device only; a call captures into a HIP graph and a replay
 * reads the lengths held then.  The rule:
 * sage_attn_tile_mass_kvlen
 *   - Operands: k8 and k_scale as sage_k_smooth_quant_kvlen makes them (statistics over the rows < len_b), q8 and q_scale
 *     as for the twin (Q has no lengths).
 *   - For every b with len_b > 0, mass[b, :, :, :ntk_b] is BIT-IDENTICAL to the twin called on q8[b:b+1], k8[b:b+1, :, :len_b]
 *     and their scales (N = len_b) with the same granularity: the softmax runs over the keys < len_b, tile ntk_b - 1 is masked
 *     at len_b, and both passes add in the order of the twin, over fewer tiles.
 *   - The entries [ntk_b, ceil(N/64)) are exactly 0, and every entry of mass is written by every call.  A batch with
 *     len_b == 0 has an all-zero row: the one exception to "every mass[b,h,i,:] sums to 1".
 *   - Nothing in rows >= len_b of k8 and no scale of a tile >= ntk_b influences anything -- they are never loaded.
 * sage_block_plan_recall_kvlen
 *   - recall[b,h,i] = sum of mass[b,h,i,j] over the listed tiles j < ntk_b, kept[b,h,i] = the number of those entries.
 *   - The sum runs in the tile slots and the fixed tree of the twin, so it is BIT-IDENTICAL to the twin on the lists of the
 *     map cut to ntk_b columns and the mass cut likewise, and as monotone under set inclusion.
 *   - The clip is by list entry and does not rely on mass being 0 beyond the length.  The lists are read-only: lists made
 *     without lengths (sage_block_map_compact, sage_block_select) serve any lengths, as do those of sage_block_select_kvlen,
 *     which hold no entry >= ntk_b in the first place.  A batch with len_b == 0 has recall 0 and kept 0. */
int sage_attn_tile_mass_kvlen(const sage_tensor* q8, const sage_tensor* k8, const float* q_scale, const float* k_scale,
                              int B, int Hq, int Hk, int M, int N, int D, int qk_gran, int blkq, int warpq,
                              float sm_scale, int logit_mult_is_one, float* mass, const int32_t* kv_lens,
                              sage_stream_t stream);
int sage_block_plan_recall_kvlen(const int32_t* block_lists, int64_t block_lists_bytes, const float* mass, int B, int Hq,
                                 int M, int N, float* recall, int32_t* kept, const int32_t* kv_lens, sage_stream_t stream);

/* ==== split-KV attention (new: few query rows against many keys -- text or latent queries over a long video context, a
 * decode step or a speculative chunk over a padded KV cache.  Every other attention entry point launches one workgroup per
 * (b, h_q, 128-row q-block) that walks all key tiles of its head; with M = 1..1024 and N = 16K..128K that grid leaves most of
 * the chip idle.  Here S = num_splits workgroups share the keys of a q-block and a second launch merges their results) ====
 * Inputs: the padded [B,H,N,D] operands of sage_attn_fusedq_pv_{f16,f8} (K quantized with its smoothing mean km), an optional
 * kv_lens (device, int32 [B], 4-byte aligned, NULL = every batch has N keys), 1 <= num_splits <= SAGE_MERGE_MAX.  The rule:
 *   - Key ranges.  len_b = clamp(kv_lens[b], 0, N), or N without kv_lens; ntk_b = ceil(len_b / 64); tps_b = ceil(ntk_b / S).
 *     Split s of batch b owns the key tiles [s * tps_b, min((s + 1) * tps_b, ntk_b)); the last valid tile is masked at len_b.
 *     A split whose range is empty takes no part: the batch has ceil(ntk_b / tps_b) non-empty splits (0 when len_b == 0), the
 *     first ones.  The merge computes this count itself; an empty split writes nothing, and nothing is read from its slot.
 *   - Statistics are those of the whole call: km, the K scales and the FP8 v_scale are what sage_k_smooth_quant /
 *     sage_kv_prepare_fp8 (with kv_lens: their _kvlen twins) make of all the keys.  All splits share one smoothing vector.
 *   - Partial result of split s: the state of the attention loop run over exactly its tiles, in ascending order, from the
 *     empty state.  The normalised row o_s is stored in fp32, before any rounding to the output type, into the workspace
 *     ([S,B,Hq,M,D] fp32), its raw base-2 LSE lse2_s behind it ([S,B,Hq,M] fp32).  o_s rounded to o_dtype (nearest even) is
 *     BIT-IDENTICAL to the o of sage_attn_fusedq_pv_*_blocksparse(_kvlen) called with lists that hold exactly those tile
 *     columns in every q-block -- which in turn is bit-identical to the dense 4-wave kernel on the gathered tiles.
 *   - Final result: with mx = max_s lse2_s and w_s = 2^(lse2_s - mx) over the non-empty splits in split order,
 *     o = (sum_s w_s o_s) / (sum_s w_s), rounded ONCE to o_dtype, and lse = (mx + log2(sum_s w_s)) / log2(e) +
 *     (q . km) * sm_scale, the smoothing correction added once.  No atomics: two calls give the same bits.
 *   - len_b == 0: o = 0, lse = -inf.  Nothing in rows >= len_b of K or V influences any output, NaN and Inf included.
 *   - The lengths are read on the device only: no host synchronisation, no pointer arrays; both launches capture into a HIP
 *     graph, and a replay reads the lengths the buffer holds then.
 * The arguments of sage_attn_fusedq_pv_{f16,f8} without is_causal, then kv_lens (may be NULL), num_splits, workspace (16-byte
 * aligned, at least sage_splitkv_workspace_bytes(B, Hq, M, D, num_splits) bytes; contents unspecified afterwards, slots of
 * empty splits untouched) and workspace_bytes.  lse may be NULL.  Always 4-wave workgroups (SAGE_TUNE_NWAVES does not apply).
 * Checked before the first launch: num_splits outside [1, SAGE_MERGE_MAX], workspace NULL, unaligned or too small, kv_lens
 * misaligned -> SAGE_ERR_INVALID_ARGUMENT; the 2 GiB slice window and every other argument as sage_attn_fusedq_pv_*.
 * Not built, SAGE_ERR_UNSUPPORTED: SAGE_GRAN_PER_BLOCK, v_mean != NULL (V smoothing), km == NULL (K smoothing off) or
 * misaligned.  There is no causal form (the library's causal mask is top-left aligned: with M << N it would mask nearly every
 * key), no block map, attn_mask, cu_seqlens or kv_layout form, no INT8-Q form, no 8-wave geometry and no one-call operator. */
size_t sage_splitkv_workspace_bytes(int B, int Hq, int M, int D, int num_splits); /* 0 for arguments out of range */
int sage_attn_fusedq_pv_f16_splitkv(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v,
                                    int v_dtype, const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                    const float* v_mean, float* lse, int B, int Hq, int Hk, int M, int N, int D,
                                    int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens, int num_splits,
                                    void* workspace, size_t workspace_bytes, sage_stream_t stream);
int sage_attn_fusedq_pv_f8_splitkv(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_fp8,
                                   const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                   const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                   int N, int D, int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens,
                                   int num_splits, void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ==== causal split-KV attention (new: a speculative chunk, a multi-token decode step, a chunk of a chunked prefill over a
 * padded KV cache.  The causal mask of every other entry point is top-left aligned -- row i sees keys 0..i -- which with
 * M << N masks nearly every key.  Here the M query rows are the LAST tokens of the batch's valid keys: the alignment that
 * FlashAttention calls bottom-right, with a diagonal that moves with kv_lens[b] on the device) ====
 * Inputs and workspace: those of sage_attn_fusedq_pv_{f16,f8}_splitkv, and a fold q_fold = g >= 1 that divides M.  The rule:
 *   - len_b = clamp(kv_lens[b], 0, N), or N without kv_lens.  The M rows are T = M / g tokens of g rows each, token-major:
 *     row r is token t = r / g (with grouped-query attention, the g = Hq / Hk query heads of a KV head folded into rows:
 *     [B,Hq,T,D] -> [B,Hk,T*g,D], row t*g + i = head i of token t).  off_b = len_b - T; it may be negative.
 *   - Row r attends the keys j with 0 <= j <= t + off_b (which implies j < len_b).  A row with t + off_b < 0 has no key --
 *     the chunk is longer than what the cache holds -- and gets o = 0, lse = -inf.  len_b == 0: o = 0, lse = -inf everywhere.
 *   - Split ranges, statistics, partial results and the merge arithmetic are exactly those of the non-causal form above:
 *     split s owns the tiles [s * tps_b, min((s + 1) * tps_b, ntk_b)); km, the K scales and the FP8 v_scale are those of the
 *     length-aware pre-pass of the whole call (padding rows influence nothing, NaN included); the merge runs in split order
 *     without atomics, and two calls give the same bits.  A split in which a row keeps no key takes no part in that row's sums.
 *   - Which workgroups run.  For q-block qb (128 rows) let end_qb = min(len_b, floor(min(128 qb + 127, M - 1) / g) + off_b + 1),
 *     the key bound of its last row.  Workgroup (b, h, qb, s) runs iff 64 * s * tps_b < end_qb.  The merge derives the same
 *     count per q-block, min(ceil(ntk_b / tps_b), ceil(ceil(end_qb / 64) / tps_b)) (0 for end_qb <= 0), and loads no slot at
 *     or beyond it; a q-block with count 0 gets o = 0, lse = -inf, and the merge reads neither the workspace nor the parked
 *     q . km correction for it.
 *   - num_splits = 1 is valid and runs this kernel with one split: there is no dense operator with this alignment.
 *   - T = 1, g = 1 is the non-causal form: the one token sees every valid key, and o and lse have its bits.
 * The arguments of sage_attn_fusedq_pv_{f16,f8}_splitkv with q_fold inserted after num_splits.  q_fold < 1 or M % q_fold != 0
 * -> SAGE_ERR_INVALID_ARGUMENT; everything the non-causal form refuses is refused here with the same status. */
int sage_attn_fusedq_pv_f16_splitkv_causal(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v,
                                           int v_dtype, const sage_tensor* o, int o_dtype, const float* k_scale,
                                           const void* km, const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                           int N, int D, int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens,
                                           int num_splits, int q_fold, void* workspace, size_t workspace_bytes,
                                           sage_stream_t stream);
int sage_attn_fusedq_pv_f8_splitkv_causal(const sage_tensor* q, int q_dtype, const sage_tensor* k8, const sage_tensor* v_fp8,
                                          const sage_tensor* o, int o_dtype, const float* k_scale, const void* km,
                                          const float* v_scale, const float* v_mean, float* lse, int B, int Hq, int Hk, int M,
                                          int N, int D, int qk_gran, int warpq, float sm_scale, const int32_t* kv_lens,
                                          int num_splits, int q_fold, void* workspace, size_t workspace_bytes,
                                          sage_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SAGEATTN_HIP_H */
