// One-call operators: everything sageattn_qk_int8_pv_fp16_cuda / sageattn_qk_int8_pv_fp8_cuda do below their argument
// checks (core.py:604-651, 786-905) behind ONE C-ABI crossing and ONE caller-provided workspace -- K mean + INT8 K
// (sage_k_smooth_quant / sage_kv_prepare_fp8), FP8 V, Q quantizer (folded into the attention kernel's prologue unless
// fuse_q = 0), attention, LSE fix.  Host code only: it checks every step with the entry points' own checks (sage_entry.h)
// and then launches them on the caller's stream, so the results are bit-identical to calling them one by one (what the
// Python mirror did until round 3: 3-4 crossings and 6-9 allocations per call, 46 us of host time against a 64 us GPU step
// at (4,32,1024,64)).
#include "sage_entry.h"

namespace {

constexpr size_t kAlign = 256;
inline size_t up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

struct Plan {
  bool fuse_q;
  size_t k8, ks, km, pre_ws, v8, v_scale, q8, qs, corr, lse2, total;  // byte offsets (valid where the piece exists)
  int gk, gq, npad;
};

// `a`: pv_fp8 and the shape
bool make_plan(Plan& pl, const sage::AttnArgs& a, bool want_lse, const sage_op_opts* o) {
  const int B = a.B, Hq = a.Hq, Hk = a.Hk, M = a.M, N = a.N, D = a.D;
  if (B <= 0 || Hq <= 0 || Hk <= 0 || M <= 0 || N <= 0 || (D != 64 && D != 128) || !o) return false;
  const int gran = o->qk_gran, warpq = o->warpq ? o->warpq : 32;
  if (gran != SAGE_GRAN_PER_WARP && gran != SAGE_GRAN_PER_THREAD) return false;
  if (warpq != 16 && warpq != 32) return false;
  pl.fuse_q = o->fuse_q != 0;  // -1 (the library's choice) = fused: it is at least as fast at every length (core.py, round 3)
  pl.npad = (N + 63) / 64 * 64;
  pl.gk = (N + 63) / 64 * (gran == SAGE_GRAN_PER_THREAD ? 4 : 1);
  const int nblkq = (M + 127) / 128;
  pl.gq = gran == SAGE_GRAN_PER_WARP ? nblkq * (128 / warpq) : nblkq * (128 / warpq) * 8;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += up(bytes); return at; };
  pl.k8 = take((size_t)B * Hk * N * D);
  pl.ks = take((size_t)B * Hk * pl.gk * 4);
  pl.km = take((size_t)B * Hk * D * 2);
  const size_t pre = a.pv_fp8 ? sage_kv_prepare_fp8_workspace_bytes(B, Hk, N, D) : sage_k_mean_workspace_bytes(B, Hk, N, D);
  pl.pre_ws = take(pre > 4 ? pre : 4);
  pl.v8 = pl.v_scale = 0;
  if (a.pv_fp8) {
    pl.v8 = take((size_t)B * Hk * D * pl.npad);
    pl.v_scale = take((size_t)B * Hk * D * 4);
  }
  pl.q8 = pl.qs = pl.corr = pl.lse2 = 0;
  if (!pl.fuse_q) {
    pl.q8 = take((size_t)B * Hq * M * D);
    pl.qs = take((size_t)B * Hq * pl.gq * 4);
    if (want_lse) {
      pl.corr = take((size_t)B * Hq * M * 4);
      pl.lse2 = take((size_t)B * Hq * M * 4);
    }
  }
  pl.total = off;
  return true;
}

// `aa` arrives with what the caller gave -- q, v and o in `dtype`, pv_fp8, lse, the shape, is_causal, sm_scale -- and leaves as
// the arguments of the attention step
int run(sage::AttnArgs aa, const sage_tensor* k, int dtype, float scale_max, const sage_op_opts* opts, void* workspace,
        size_t workspace_bytes, sage_stream_t stream) {
  const sage_tensor *const q = aa.q, *const v = aa.v;
  float* const lse = aa.lse;
  const int pv_fp8 = aa.pv_fp8, B = aa.B, Hq = aa.Hq, Hk = aa.Hk, M = aa.M, N = aa.N, D = aa.D;
  if (!q || !k || !v || !aa.o || !opts || !workspace) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = sage::dim_dtype_status(D, dtype)) return s;
  if (Hk <= 0 || Hq % Hk != 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (!opts->smooth_k) return SAGE_ERR_UNSUPPORTED;  // the un-smoothed variant goes through the separate entry points
  if (opts->nwaves != 0 && opts->nwaves != 4 && opts->nwaves != 8) return SAGE_ERR_INVALID_ARGUMENT;
  Plan pl;
  if (!make_plan(pl, aa, lse != nullptr, opts)) return SAGE_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < pl.total || !sage::aligned16(workspace)) return SAGE_ERR_INVALID_ARGUMENT;
  char* const ws = static_cast<char*>(workspace);
  const int gran = opts->qk_gran, warpq = opts->warpq ? opts->warpq : 32;
  const int rounding = gran == SAGE_GRAN_PER_THREAD ? SAGE_ROUND_TRITON : SAGE_ROUND_CUDA;      // core.py:621-624
  const int k_gran = gran == SAGE_GRAN_PER_THREAD ? SAGE_GRAN_PER_THREAD : SAGE_GRAN_PER_BLOCK;  // per_warp: K per block
  // internal operands are head-major whatever the caller's layout: the attention kernel then streams the rows of one
  // head from consecutive lines
  const sage_tensor k8{ws + pl.k8, (int64_t)Hk * N * D, (int64_t)N * D, D};
  float* const ks = reinterpret_cast<float*>(ws + pl.ks);
  void* const km = ws + pl.km;
  sage_tensor v8{nullptr, 0, 0, 0};
  float* v_scale = nullptr;
  // every step is checked before the first launch: K (+ V) pre-pass, Q quantizer (fuse_q = 0), attention, LSE fix
  sage::KSmoothCall kc;
  sage::KVPrepCall kvc;
  int st;
  if (pv_fp8) {
    v8 = sage_tensor{ws + pl.v8, (int64_t)Hk * D * pl.npad, (int64_t)D * pl.npad, pl.npad};
    v_scale = reinterpret_cast<float*>(ws + pl.v_scale);
    st = sage::kv_prepare_check(kvc, k, v, dtype, B, Hk, N, D, &k8, ks, km, k_gran, rounding, &v8, v_scale, scale_max,
                                ws + pl.pre_ws);
  } else {
    st = sage::k_smooth_quant_check(kc, k, dtype, B, Hk, N, D, &k8, ks, km, k_gran, rounding, ws + pl.pre_ws);
  }
  if (st != SAGE_OK) return st;
  // the attention step reads the pre-pass results; Q: the fp16 / bf16 tensor (fused), or q8 and its scales
  aa.k8 = &k8; aa.k_scale = ks; aa.v_scale = v_scale; aa.v_dtype = pv_fp8 ? SAGE_F16 : dtype; aa.o_dtype = dtype;
  if (pv_fp8) aa.v = &v8;
  aa.qk_gran = gran; aa.blkq = 128; aa.warpq = warpq; aa.nwaves = opts->nwaves;
  sage::AttnCall ac;
  sage::QuantCall qc;
  sage::FinishLseCall fc;
  const sage_tensor q8{ws + pl.q8, (int64_t)Hq * M * D, (int64_t)M * D, D};
  if (pl.fuse_q) {
    aa.q_dtype = dtype; aa.km = km;
    st = sage::attn_check(ac, aa);
  } else {
    float* const qs = reinterpret_cast<float*>(ws + pl.qs);
    float* const corr = lse ? reinterpret_cast<float*>(ws + pl.corr) : nullptr;
    float* const lse2 = lse ? reinterpret_cast<float*>(ws + pl.lse2) : nullptr;
    st = sage::quant_check(qc, q, dtype, B, Hq, M, D, nullptr, &q8, qs, gran, 0, 128, warpq, 1.0f, rounding, lse ? km : nullptr,
                           Hq / Hk, corr);
    aa.q = &q8; aa.q_scale = qs; aa.lse = lse2;
    if (st == SAGE_OK) st = sage::attn_check(ac, aa);
    if (st == SAGE_OK && lse) st = sage::finish_lse_check(fc, lse2, corr, aa.sm_scale, lse, (int64_t)B * Hq * M);
  }
  if (st != SAGE_OK) return st;
  const hipStream_t s = (hipStream_t)stream;
  st = pv_fp8 ? sage::kv_prepare_launch(kvc, s) : sage::k_smooth_quant_launch(kc, s);
  if (st == SAGE_OK && !pl.fuse_q) st = sage::quant_launch(qc, s);
  if (st == SAGE_OK) st = sage::attn_launch(ac, s);
  if (st == SAGE_OK && !pl.fuse_q && lse) st = sage::finish_lse_launch(fc, s);
  return st;
}

}  // namespace

extern "C" size_t sage_sageattn_workspace_bytes(int pv_fp8, int B, int Hq, int Hk, int M, int N, int D, int want_lse,
                                                const sage_op_opts* opts) {
  sage::AttnArgs a;
  a.pv_fp8 = pv_fp8 != 0; a.B = B; a.Hq = Hq; a.Hk = Hk; a.M = M; a.N = N; a.D = D;
  Plan pl;
  return make_plan(pl, a, want_lse != 0, opts) ? pl.total : 0;
}

extern "C" int sage_sageattn_pv_f16(const sage_tensor* q, const sage_tensor* k, const sage_tensor* v, int dtype,
                                    const sage_tensor* o, float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal,
                                    float sm_scale, const sage_op_opts* opts, void* workspace, size_t workspace_bytes,
                                    sage_stream_t stream) {
  sage::AttnArgs a;
  a.q = q; a.v = v; a.o = o; a.lse = lse; a.B = B; a.Hq = Hq; a.Hk = Hk; a.M = M; a.N = N; a.D = D; a.is_causal = is_causal;
  a.sm_scale = sm_scale;
  return run(a, k, dtype, 0.f, opts, workspace, workspace_bytes, stream);
}

extern "C" int sage_sageattn_pv_f8(const sage_tensor* q, const sage_tensor* k, const sage_tensor* v, int dtype,
                                   const sage_tensor* o, float* lse, int B, int Hq, int Hk, int M, int N, int D, int is_causal,
                                   float sm_scale, float scale_max, const sage_op_opts* opts, void* workspace,
                                   size_t workspace_bytes, sage_stream_t stream) {
  if (!(scale_max > 0.f)) return SAGE_ERR_INVALID_ARGUMENT;
  sage::AttnArgs a;
  a.q = q; a.v = v; a.pv_fp8 = true; a.o = o; a.lse = lse; a.B = B; a.Hq = Hq; a.Hk = Hk; a.M = M; a.N = N; a.D = D;
  a.is_causal = is_causal; a.sm_scale = sm_scale;
  return run(a, k, dtype, scale_max, opts, workspace, workspace_bytes, stream);
}
