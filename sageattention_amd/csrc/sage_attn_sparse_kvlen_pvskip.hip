// Block-sparse attention with the P.V skip and per-batch key lengths: the loop body of sage_attn.hip with SPARSE, PVSKIP and
// KVLEN.  What the lengths add is described in sage_attn_sparse_kvlen.hip, what the skip adds in sage_attn_pvskip.hip.  A
// source file of its own because, like the latter, it is compiled with -mllvm -structurizecfg-skip-uniform-regions
// (sageattention_amd/_build.py): without the option the wave-uniform skip branch costs +36 ... +40 vector registers.
#include "sage_attn_launch.h"

namespace sage {

template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
// (register budget as attn_i8_blocksparse_pvskip_kernel: the two bf16-V variants at head_dim 64 run at two waves per SIMD)
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_blocksparse_pvskip_kvlen_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = false, HAS_MASK = false, SPARSE = true, PVSKIP = true, KVLEN = true, SPLITKV = false, PAGED = false;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

int launch_blocksparse_pvskip_kvlen(const AttnCall& c, hipStream_t st) {
  return launch_4wave_kernel(c, st, c.p.nqb * c.p.Hq * c.p.B, [](auto d, auto k, auto v, auto fp8) {
    return attn_i8_blocksparse_pvskip_kvlen_kernel<decltype(d)::value, decltype(k)::value, decltype(v)::value, decltype(fp8)::value>;
  });
}

}  // namespace sage
