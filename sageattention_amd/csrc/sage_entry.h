// The check and launch halves of the entry points that the one-call operators (sage_op.hip) chain.  Every C-ABI entry point
// checks all its arguments and fills its kernel parameters, with no HIP call, before its first launch, and then launches
// with no further check: a call that returns an argument status has enqueued nothing.  sage_op.hip checks every step of a
// call with these functions before it launches the first step.
#pragma once
#include "sage_attn_common.h"  // AttnParams

namespace sage {

// ---- INT8 quantizer (sage_quant.hip) ----------------------------------------------------------------------------------
struct QuantParams {
  const uint16_t* x;
  int64_t xsb, xsh, xsn;
  const uint16_t* mean;  // [B,H,D] or null
  int8_t* out;
  int64_t osb, osh, osn;
  float* scale;  // [B,H,G]
  const uint16_t* dot_vec;  // [B,H/dot_group,D] or null
  float* dot_out;           // [B,H,N]
  int dot_group;
  int N, G;          // rows, scales per (b,h)
  int gran, is_key;  // sage_qk_gran, K-side grouping of per_thread
  int warp;          // rows per warp group (16, 32, 64 or 128)
  int warp_shift;    // log2(warp): the group maps run per row and must not cost an integer division
  float mult;
  int rounding;
  const int* cu;  // varlen: sequence b = rows [cu[b], cu[b+1]) of the packed tensor (stride_b unused); N = max length
  // result layout: rows of block `blk` start at blk * o_blk (elements; dense: BLK * osn); scales of (b, h, blk) at
  // b*ss_b + h*ss_h + blk*ss_blk (floats; dense: [B,H,G])
  int64_t o_blk, ss_b, ss_h, ss_blk;
  // mean given as the per-chunk column sums of k_mean_partial_kernel ([B*H][S][D] fp32) instead of `mean`: the kernel
  // finishes the reduction itself (S <= 16: a few KB per workgroup out of L2) and block 0 stores km -- one launch less
  const float* mean_part;
  int S;
  uint16_t* km_out;
};

// V half of the fused K/V pre-pass (sage_quant.hip, kv_quant_kernel / kv_quant_stream_kernel)
struct VPrepParams {
  const uint16_t* v;
  int64_t sb, sh, sn;
  uint8_t* out;
  int64_t ob, oh, od, o_tile;
  float* v_scale;      // [B,H,D]
  const float* part;   // [B,H,S,D] max|v| per chunk
  float scale_max;
};

// the inputs of quant_check that only some entry points have
struct QuantOptions {
  const int* cu = nullptr;                 // packed sequences (sage_quant_qk_int8_varlen)
  int64_t out_blk_stride = 0;              // tile-major output (sage_quant_k_int8_kvtiles): elements between 64-row blocks,
  const int64_t* scale_strides = nullptr;  // and the scale strides per batch, head and block; 0 / null = dense
  const float* mean_part = nullptr;        // the mean as S chunk sums of k, finished by the quantizer, which stores it to km_out
  int S = 0;
  void* km_out = nullptr;
};

// one launch of quant_qk_int8_kernel
struct QuantCall {
  QuantParams p;
  int B, H, D, blk;
  bool bf16;
};
int quant_check(QuantCall& c, const sage_tensor* x, int dtype, int B, int H, int N, int D, const void* mean,
                const sage_tensor* out, float* scale, int gran, int is_key, int blk, int warp, float mult, int rounding,
                const void* lse_dot_vec, int dot_group, float* lse_dot, const QuantOptions& opt = QuantOptions());
int quant_launch(const QuantCall& c, hipStream_t st);

// sage_k_smooth_quant: chunk sums of k into the workspace (q.p.mean_part), then the streaming quantizer
struct KSmoothCall {
  QuantCall q;
  sage_tensor k;
  float* part;
  int per_wg;  // 64-row blocks per workgroup of the quantizer
  const int32_t* kv_lens = nullptr;  // sage_k_smooth_quant_kvlen: rows >= clamp(kv_lens[b], 0, N) of batch b are absent
  int slots;   // chunk slots per head of `part`: the chunks of N rows, with kv_lens the most a batch of up to N rows can have
};
int k_smooth_quant_check(KSmoothCall& c, const sage_tensor* k, int dtype, int B, int H, int N, int D, const sage_tensor* out,
                         float* scale, void* km, int gran, int rounding, void* workspace, const int32_t* kv_lens = nullptr);
int k_smooth_quant_launch(const KSmoothCall& c, hipStream_t st);

// sage_kv_prepare_fp8: K and V chunk statistics, then both quantizers in one launch
struct KVPrepCall {
  QuantCall k;
  VPrepParams v;
  float* kpart;
  float* vpart;
  int nblk_k, nunit_v;  // K blocks, V units (VQuantGeom<D>::BLKS blocks each)
  int per_k, per_v;     // ... per workgroup of the streaming kernel
  bool streaming;       // kv_quant_stream_kernel, else kv_quant_kernel (one block / unit per workgroup)
  const int32_t* kv_lens = nullptr;  // sage_kv_prepare_fp8_kvlen: rows >= clamp(kv_lens[b], 0, N) of batch b are absent
  int slots;            // chunk slots per head of kpart and vpart (as KSmoothCall::slots)
};
int kv_prepare_check(KVPrepCall& c, const sage_tensor* k, const sage_tensor* v, int dtype, int B, int H, int N, int D,
                     const sage_tensor* k_int8, float* k_scale, void* km, int gran, int rounding, const sage_tensor* v_fp8,
                     float* v_scale, float scale_max, void* workspace,
                     const int32_t* kv_lens = nullptr);
int kv_prepare_launch(const KVPrepCall& c, hipStream_t st);

// ---- attention (sage_attn.hip) ----------------------------------------------------------------------------------------
// the arguments of an attention entry point: each one names the fields it has and leaves the others at these defaults
struct AttnArgs {
  const sage_tensor *q = nullptr, *k8 = nullptr, *v = nullptr, *o = nullptr;  // q: INT8, or with q_dtype >= 0 fp16 / bf16
  bool pv_fp8 = false;                                                        // v is the FP8 V^T, else fp16 / bf16 (v_dtype)
  int v_dtype = SAGE_F16, o_dtype = SAGE_F16;
  const float *q_scale = nullptr, *k_scale = nullptr, *v_scale = nullptr, *v_mean = nullptr;
  float* lse = nullptr;
  int B = 0, Hq = 0, Hk = 0, M = 0, N = 0, D = 0;
  int is_causal = 0, qk_gran = 0, blkq = 0, warpq = 0;
  float sm_scale = 0.f;
  int logit_mult_is_one = 0;
  const int *cu_q = nullptr, *cu_k = nullptr;  // packed sequences: cumulative query / key lengths
  int q_dtype = -1;           // >= 0: q is the fp16 / bf16 query tensor, quantized in the kernel's prologue
  const void* km = nullptr;   // fused Q: k_mean of the LSE correction
  const void* mask = nullptr; // attn_mask, its kind and its four strides
  int mask_kind = 0;
  const int64_t* mask_strides = nullptr;
  const sage_kv_layout* kvl = nullptr;  // tile-major K / V buffers
  int nwaves = 0;             // waves per workgroup (4 or 8); 0 = the thread's SAGE_TUNE_NWAVES if set, else the measured choice
  bool block_sparse = false;  // block-sparse form: the tile lists of sage_block_map_compact and the size of their buffer
  const int32_t* block_lists = nullptr;
  int64_t block_lists_bytes = 0;
  bool pv_skip = false;       // ... with the P.V skip: per-head thresholds (fp32 [Hq]) and the skip counters (or null)
  const float* pv_thresh = nullptr;
  int32_t* pv_skipped = nullptr;
  bool key_lens = false;      // per-batch key lengths: batch b attends its keys [0, clamp(kv_lens[b], 0, N)) (device, int32 [B])
  const int32_t* kv_lens = nullptr;
  // per-batch key lengths of the BLOCK-SPARSE form (with or without pv_skip): a field of its own.  key_lens above keeps
  // meaning "the dense kernel with lengths" and stays SAGE_ERR_UNSUPPORTED together with block_sparse; the lists of this form
  // are clipped at ceil(len_b / 64) tiles by the kernel (sage_attn_sparse_kvlen.hip).  Same tensor: device, int32 [B]
  bool block_key_lens = false;
  const int32_t* block_kv_lens = nullptr;
  // split-KV (sage_attn_fusedq_pv_*_splitkv, fused Q only): num_splits workgroups per (b, h, q-block), each on its range of
  // key tiles, then the merge of their fp32 partial results out of the caller's workspace.  Its key lengths are a field of
  // its own and OPTIONAL (null: every batch has N keys); with key_lens, a block map, causal, attn_mask, cu_seqlens, a
  // kv_layout or v_mean: SAGE_ERR_UNSUPPORTED
  bool split_kv = false;
  const int32_t* split_kv_lens = nullptr;
  int num_splits = 0;
  void* split_workspace = nullptr;
  size_t split_workspace_bytes = 0;
  // ... causal (sage_attn_fusedq_pv_*_splitkv_causal), a field of its own: is_causal above keeps meaning the top-left mask
  // of the dense kernels and stays SAGE_ERR_UNSUPPORTED together with split_kv.  The M rows are M / q_fold tokens, the last
  // positions of the batch's keys; q_fold < 1 or M % q_fold != 0: SAGE_ERR_INVALID_ARGUMENT
  bool split_causal = false;
  int q_fold = 1;
  // ... paged (sage_attn_fusedq_pv_*_splitkv_paged, include/sageattn_hip_paged.h; with split_kv only, else
  // SAGE_ERR_UNSUPPORTED): k8, v and k_scale are pools of pages -- stride_b of k8 and v is the stride of a page -- and row b of
  // block_table (int32, table_stride entries per row) names the pages of batch b; page_size is 64, 128 or 256 keys and N the
  // logical capacity max_pages * page_size.  The entry point checks the table's own arguments; here the 32-bit window is that
  // of one (page, head) slice and the K scales are laid out per page
  bool paged = false;
  const int32_t* block_table = nullptr;
  int table_stride = 0, page_size = 0;
};

// one launch of attn_i8_kernel: its parameters and the template arguments they select
struct AttnCall {
  AttnParams p;
  int D, nwaves;
  bool pv_fp8, causal, kthread, v_bf16;
  bool sparse;  // attn_i8_blocksparse_kernel (always 4 waves)
  bool pvskip;  // ... its twin attn_i8_blocksparse_pvskip_kernel
  bool kvlen;   // attn_i8_kvlen_kernel: the dense kernel with per-batch key lengths
  bool sparse_kvlen;  // attn_i8_blocksparse_kvlen_kernel / ..._pvskip_kvlen_kernel: sparse (and pvskip) with key lengths
  bool splitkv;  // attn_i8_splitkv_kernel + splitkv_merge_kernel (always 4 waves)
  bool splitkv_causal;  // ... attn_i8_splitkv_causal_kernel + splitkv_merge_kernel<.., CAUSAL = true>, with splitkv
  bool paged;  // ... attn_i8_splitkv_paged_kernel / attn_i8_splitkv_causal_paged_kernel in the place of the two, with splitkv
};
int attn_check(AttnCall& c, const AttnArgs& a);
int attn_launch(const AttnCall& c, hipStream_t st);
// the attention launch of a block-sparse call with the P.V skip (c.pvskip; sage_attn_pvskip.hip): attn_launch goes through it
int launch_blocksparse_pvskip(const AttnCall& c, hipStream_t st);
// the attention launch of a call with per-batch key lengths (c.kvlen; sage_attn_kvlen.hip): attn_launch goes through it
int launch_kvlen(const AttnCall& c, hipStream_t st);
// the launches of a block-sparse call with per-batch key lengths (c.sparse_kvlen; sage_attn_sparse_kvlen.hip): the attention
// kernel -- with c.pvskip the twin of sage_attn_sparse_kvlen_pvskip.hip, second function -- and the rows of the emptied q-blocks
int launch_blocksparse_kvlen(const AttnCall& c, hipStream_t st);
int launch_blocksparse_pvskip_kvlen(const AttnCall& c, hipStream_t st);
// the launches of a split-KV call (c.splitkv), which attn_launch makes in this order: the attention kernel over the splits --
// sage_attn_splitkv.hip, or with c.splitkv_causal its twin of sage_attn_splitkv_causal.hip -- then the merge of either form
// (sage_attn_splitkv.hip)
int launch_splitkv_attn(const AttnCall& c, hipStream_t st);
int launch_splitkv_causal_attn(const AttnCall& c, hipStream_t st);
int launch_splitkv_merge(const AttnCall& c, hipStream_t st);
// ... of a paged split-KV call (c.paged; sage_attn_splitkv_paged.hip / sage_attn_splitkv_causal_paged.hip): the attention
// kernel in the place of the two above, then the same merge
int launch_splitkv_paged_attn(const AttnCall& c, hipStream_t st);
int launch_splitkv_causal_paged_attn(const AttnCall& c, hipStream_t st);
// ... of a shared-prefix call (include/sageattn_hip_prefix.h; sage_attn_prefix.hip), which goes through the two launches above
// itself -- attn_launch would append the merge of ONE segment -- and then through this one: the merge of the prefix call's and
// the suffix call's partial slots, each segment with the correction its split 0 parked at c.p.lse, into suffix.p.o and `lse`
int launch_prefix_merge(const AttnCall& prefix, const AttnCall& suffix, float* lse, hipStream_t st);
// bytes of the workspace of a split-KV call: the partial outputs fp32 [S,B,Hq,M,D], then their base-2 LSEs fp32 [S,B,Hq,M]
inline int64_t splitkv_bytes(int B, int Hq, int M, int D, int S) {
  return (int64_t)S * B * Hq * M * ((int64_t)D + 1) * 4;
}

// ---- block-sparse tile lists (sage_misc.hip) ---------------------------------------------------------------------------
// bytes of the lists of one call: a row of block_list_row(N) int32 per (b, h_q, 128-row q-block)
inline int64_t block_sparse_bytes(int B, int Hq, int M, int N) {
  return (int64_t)B * Hq * (((int64_t)M + 127) / 128) * block_list_row(N) * 4;
}

// ---- sage_finish_lse (sage_misc.hip) ------------------------------------------------------------------------------------
struct FinishLseCall {
  const float* lse2;
  const float* corr;
  float sm_scale;
  float* out;
  int64_t n;
};
int finish_lse_check(FinishLseCall& c, const float* lse2, const float* corr, float sm_scale, float* lse_out, int64_t n);
int finish_lse_launch(const FinishLseCall& c, hipStream_t st);

}  // namespace sage
