// Block-sparse attention with SpargeAttn's second stage, the P.V skip (the rule: include/sageattn_hip.h,
// sage_attn_*_blocksparse_pvskip): the loop body of sage_attn.hip with PVSKIP = true.  A wave leaves out the softmax and the
// P.V of a tile whose scores all lie at least pv_thresh[h] below the running maximum of their rows, and reports how many
// tiles it skipped.
//
// A kernel of its own name, not a template parameter of attn_i8_blocksparse_kernel: the build's occupancy guard matches that
// kernel's mangled name, and the instantiations without the skip keep their code.  A source file of its own, because it is
// compiled with -mllvm -structurizecfg-skip-uniform-regions (sageattention_amd/_build.py): the skip is a wave-uniform
// if / else around the middle of the tile, and without the option hipcc's structurizer rewrites that diamond -- uniform or
// not -- into two if-thens in a row.  The O accumulators then stay live across the computing half into the skipping one,
// the first P.V MFMA of a tile can no longer work in place, and O and the row sums get a second home: +36 ... +40 vector
// registers, i.e. two waves per SIMD at head_dim 64 and scratch at head_dim 128.  With the option the branch stays a
// scalar branch and every variant needs no more registers than its twin without the skip.  Regions with a divergent
// branch are structurized as before.
#include "sage_attn_launch.h"

namespace sage {

template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
// (head_dim 64: the FP16-V and FP8 variants stay within 168 registers = three waves per SIMD, as their twins, and the build
//  holds them to it.  The two bf16-V variants need 172 / 176 -- the branch alone costs them 6-8 registers, with an empty skip
//  path as well -- and spill when told to stay below the line: they run at two waves per SIMD)
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_blocksparse_pvskip_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = false, HAS_MASK = false, SPARSE = true, PVSKIP = true, KVLEN = false, SPLITKV = false, PAGED = false;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

int launch_blocksparse_pvskip(const AttnCall& c, hipStream_t st) {
  return launch_4wave_kernel(c, st, c.p.nqb * c.p.Hq * c.p.B, [](auto d, auto k, auto v, auto fp8) {
    return attn_i8_blocksparse_pvskip_kernel<decltype(d)::value, decltype(k)::value, decltype(v)::value, decltype(fp8)::value>;
  });
}

}  // namespace sage
