// Dense attention with per-batch key lengths (the rule: include/sageattn_hip.h, sage_attn_*_kvlen): the loop body of
// sage_attn.hip with KVLEN = true.  Batch b attends its keys [0, len_b), len_b = clamp(kv_lens[b], 0, N), on the ordinary padded
// [B,H,N,D] operands.  The body takes its key count from a per-batch variable anyway (packed sequences overwrite it): here it
// becomes len_b, one scalar load in the prologue, and the tile range, the tail mask and the K / V buffer descriptors follow it,
// so a batch runs exactly the instruction stream of the dense kernel called on its first len_b keys -- the pipelined loop, the
// fused Q quantizer, FP16 / BF16 / FP8 P.V, LSE, GQA, causal, both head dims and both workgroup geometries.  A workgroup of a
// batch without keys leaves before any barrier; the rows of such batches, o = 0 and lse = -inf, are written by a second, tiny
// launch (attn_kvlen_empty_kernel), as the rows of the empty q-blocks of a block-sparse call are.
//
// A kernel of its own name, not a template parameter of attn_i8_kernel: the build's occupancy guard matches that kernel's
// mangled name, and the instantiations without lengths keep their code and their registers.  A source file of its own, because
// it holds as many instantiations as sage_attn.hip has without attn_mask and compiles beside it.
#include "sage_attn_launch.h"

namespace sage {

template <int D, int NWAVES, bool CAUSAL, bool KTHREAD, bool V_BF16, bool PV_FP8>
// (register budget as attn_i8_kernel: head_dim 64 FP8 PV with 4 waves is held to three waves per SIMD)
__global__ __launch_bounds__(NWAVES * 64, (D == 64 && PV_FP8 && NWAVES == 4) ? 3 : 2)
void attn_i8_kvlen_kernel(const AttnParams p) {
  constexpr bool HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = true, SPLITKV = false, PAGED = false;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// The rows of the batches without keys (the attention kernel returns at once): o = 0, lse = -inf.  One workgroup per
// (b, h_q, kEmptyRows query rows) -- few workgroups, because all but those of empty batches leave after one scalar load and
// the launch is paid by every call.
constexpr int kEmptyRows = 1024;
__global__ __launch_bounds__(256) void attn_kvlen_empty_kernel(const AttnParams p, const int D) {
  const int nrb = (p.M + kEmptyRows - 1) / kEmptyRows, rb = blockIdx.x % nrb, bh = blockIdx.x / nrb;
  const int h = bh % p.Hq, b = bh / p.Hq;
  if (uniform_load_i32(p.kv_lens + b) > 0) return;  // (clamp(len, 0, N) > 0 iff len > 0)
  const int r0 = rb * kEmptyRows, rows = min(kEmptyRows, p.M - r0), per_row = D / 4;
  uint16_t* ob = p.o + b * p.osb + h * p.osh + (int64_t)r0 * p.osn;
  for (int i = threadIdx.x; i < rows * per_row; i += 256)
    *reinterpret_cast<uint2*>(ob + (int64_t)(i / per_row) * p.osn + (i % per_row) * 4) = make_uint2(0u, 0u);
  if (p.lse)
    for (int i = threadIdx.x; i < rows; i += 256) p.lse[((int64_t)b * p.Hq + h) * p.M + r0 + i] = -INFINITY;
}

template <int D, int NWAVES>
static int launch_kvlen_geom(const AttnCall& c, hipStream_t st) {
  const AttnParams& p = c.p;
  return by_flag(c.pv_fp8, [&](auto fp8) {
    constexpr bool PV_FP8 = decltype(fp8)::value;
    constexpr size_t smem = attn_lds_bytes(D, NWAVES, PV_FP8);
    return by_flag(c.causal, [&](auto ca) {
      return by_flag(c.kthread, [&](auto k) {
        return by_flag(!PV_FP8 && c.v_bf16, [&](auto v) {  // fp8 V has no bf16 flavour
          auto kern = attn_i8_kvlen_kernel<D, NWAVES, decltype(ca)::value, decltype(k)::value, !PV_FP8 && decltype(v)::value, PV_FP8>;
          if (!allow_lds((const void*)kern, smem)) return (int)SAGE_ERR_LAUNCH;
          hipLaunchKernelGGL(kern, dim3(p.nqb * p.Hq * p.B), dim3(NWAVES * 64), smem, st, p);
          return launch_status();
        });
      });
    });
  });
}

// the kernel, then the rows of the batches without keys
int launch_kvlen(const AttnCall& c, hipStream_t st) {
  const int s = by_dim(c.D, [&](auto d) {
    return c.nwaves == 8 ? launch_kvlen_geom<decltype(d)::value, 8>(c, st) : launch_kvlen_geom<decltype(d)::value, 4>(c, st);
  });
  if (s) return s;
  hipLaunchKernelGGL(attn_kvlen_empty_kernel, dim3(((c.p.M + kEmptyRows - 1) / kEmptyRows) * c.p.Hq * c.p.B), dim3(256), 0, st,
                     c.p, c.D);
  return launch_status();
}

}  // namespace sage
