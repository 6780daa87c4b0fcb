// Causal paged split-KV attention (the rule: include/sageattn_hip_paged.h): attn_i8_splitkv_causal_kernel
// (sage_attn_splitkv_causal.hip) on a KV cache stored in pages of one pool.  The body is sage_attn_body.h with CAUSAL = true,
// SPLITKV = true, PAGED = true: the diagonal aligned to the end of the batch's keys, the split ranges and the merge of the
// contiguous causal form, and the paged tile addressing of sage_attn_splitkv_paged.hip.  A wave that is done before its
// workgroup goes on staging tiles for it: those copies look their pages up like any other.
//
// A kernel of its own name and a source file of its own, as every other twin.  The entry points are those of
// sage_attn_splitkv_paged.hip (`causal`, `q_fold`), the merge that of sage_attn_splitkv.hip.
#include "sage_attn_launch.h"

namespace sage {

template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
// (register budget as attn_i8_kernel: head_dim 64 FP8 PV with 4 waves is held to three waves per SIMD)
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_splitkv_causal_paged_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = true, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true, PAGED = true;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// the attention launch over (b, h, q-block, split) of a causal paged call
int launch_splitkv_causal_paged_attn(const AttnCall& c, hipStream_t st) {
  return launch_4wave_kernel(c, st, c.p.nqb * c.p.Hq * c.p.B * c.p.num_splits, [](auto d, auto k, auto v, auto fp8) {
    return attn_i8_splitkv_causal_paged_kernel<decltype(d)::value, decltype(k)::value, decltype(v)::value, decltype(fp8)::value>;
  });
}

}  // namespace sage
