// Block-sparse attention with per-batch key lengths (the rule: include/sageattn_hip.h, sage_attn_*_blocksparse_kvlen): the loop
// body of sage_attn.hip with SPARSE = true and KVLEN = true.  Batch b attends the active tiles of its lists that lie below
// ntk_b = ceil(len_b / 64), len_b = clamp(kv_lens[b], 0, N), and the last of them is masked at len_b: the body takes the
// batch's key count from kv_lens as attn_i8_kvlen_kernel does (one scalar load; the tail mask and the K / V buffer descriptors
// follow it) and clips the count of its list row to the entries < ntk_b (a ballot count over the row, see the body).  The
// lists themselves are read-only: a plan compacted once for (B, Hq, M, N) serves any lengths.  A batch runs the instruction
// stream of attn_i8_blocksparse_kernel called on its first len_b keys with the map cut to ntk_b columns.
//
// A kernel of its own name in a file of its own, as the dense kernel with lengths and the P.V-skip twin are: the build's
// occupancy guard matches mangled names, and the kernels without lengths keep their code and their registers.  The twin with
// the P.V skip lives in sage_attn_sparse_kvlen_pvskip.hip because it needs that twin's compiler option.
#include "sage_attn_launch.h"

namespace sage {

template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
// (register budget as attn_i8_blocksparse_kernel: head_dim 64 FP8 PV is held to three waves per SIMD)
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_blocksparse_kvlen_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = false, HAS_MASK = false, SPARSE = true, PVSKIP = false, KVLEN = true, SPLITKV = false, PAGED = false;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// The rows of the q-blocks whose list has no entry below ntk_b (the attention kernel returns at once): o = 0, lse = -inf and,
// with skip counters, the four counters of the q-block = 0.  The list ascends, so `count == 0 || list[0] >= ntk_b` says it;
// a batch without keys has ntk_b = 0.  One workgroup per list row; all but the emptied ones leave after three scalar loads.
__global__ __launch_bounds__(256) void attn_blocksparse_kvlen_empty_kernel(const AttnParams p, const int D) {
  const int qb = blockIdx.x % p.nqb, bh = blockIdx.x / p.nqb;
  const int h = bh % p.Hq, b = bh / p.Hq;
  const int* row = p.bs_lists + (int64_t)blockIdx.x * p.bs_row;
  const int ntk_b = (min(max(uniform_load_i32(p.kv_lens + b), 0), p.N) + 63) >> 6;
  if (uniform_load_i32(row) > 0 && uniform_load_i32(row + 1) < ntk_b) return;
  const int rows = min(128, p.M - qb * 128), per_row = D / 4;
  uint16_t* ob = p.o + b * p.osb + h * p.osh + (int64_t)(qb * 128) * p.osn;
  for (int i = threadIdx.x; i < rows * per_row; i += 256)
    *reinterpret_cast<uint2*>(ob + (int64_t)(i / per_row) * p.osn + (i % per_row) * 4) = make_uint2(0u, 0u);
  if (p.lse && (int)threadIdx.x < rows) p.lse[((int64_t)b * p.Hq + h) * p.M + qb * 128 + threadIdx.x] = -INFINITY;
  if (p.pv_skipped && threadIdx.x < 4) p.pv_skipped[(int64_t)blockIdx.x * 4 + threadIdx.x] = 0;
}

// the kernel, or its twin with the P.V skip, then the rows of the emptied q-blocks
int launch_blocksparse_kvlen(const AttnCall& c, hipStream_t st) {
  const int grid = c.p.nqb * c.p.Hq * c.p.B;
  const int s = c.pvskip ? launch_blocksparse_pvskip_kvlen(c, st) : launch_4wave_kernel(c, st, grid, [](auto d, auto k, auto v, auto fp8) {
    return attn_i8_blocksparse_kvlen_kernel<decltype(d)::value, decltype(k)::value, decltype(v)::value, decltype(fp8)::value>;
  });
  if (s) return s;
  hipLaunchKernelGGL(attn_blocksparse_kvlen_empty_kernel, dim3(grid), dim3(256), 0, st, c.p, c.D);
  return launch_status();
}

}  // namespace sage
