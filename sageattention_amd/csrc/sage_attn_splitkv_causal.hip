// Causal split-KV attention (the rule: include/sageattn_hip.h, sage_attn_fusedq_pv_*_splitkv_causal): attn_i8_splitkv_kernel
// (sage_attn_splitkv.hip) with a diagonal that is aligned to the END of the batch's keys.  The M query rows are T = M / g
// tokens of g folded query heads each (g = q_fold; row r is token r / g), and the tokens are the last T positions of the
// batch's len_b valid keys: token t attends the keys 0 .. t + off_b, off_b = len_b - T, which moves with kv_lens[b] on the
// device.  The body is sage_attn_body.h with CAUSAL = true, SPLITKV = true: the split's range and the moved operands of the
// non-causal form, and the causal machinery of the dense kernel (wave_tiles, n_plain, mask_limit) on a per-lane limit
// `token + off_b - 64 * (first tile of the split)` in place of the row index.
//
// A row whose keys in a split are all masked: every score of it is the -inf pattern, so its row maxima are -inf, no rescale
// ever fires for it and m_run keeps its start -1e30; every p is exp2(-inf) = 0, so l_run = 0 (on the matrix pipe as well:
// a sum of zeros), inv = 1 / 0 = inf, the fp32 partial row is 0 * inf = NaN and the partial lse2 is -1e30 + log2(0) = -inf.
// The merge drops exactly such a slot by select (`l != -inf`) and never multiplies it: no per-row branch in the loop.  A row
// that keeps a key only in a LATER tile of the split starts the same way and is rescaled by alpha = exp2(-1e30 - m) = 0.
//
// A kernel of its own name and a source file of its own, as every other twin: the build's guards match kernels by name, and
// the other instantiations keep their code and their registers.  The merge, its launch and the entry points are those of
// sage_attn_splitkv.hip.
#include "sage_attn_launch.h"

namespace sage {

template <int D, bool KTHREAD, bool V_BF16, bool PV_FP8>
// (register budget as attn_i8_kernel: head_dim 64 FP8 PV with 4 waves is held to three waves per SIMD)
__global__ __launch_bounds__(256, (D == 64 && PV_FP8) ? 3 : 2)
void attn_i8_splitkv_causal_kernel(const AttnParams p) {
  constexpr int NWAVES = 4;
  constexpr bool CAUSAL = true, HAS_MASK = false, SPARSE = false, PVSKIP = false, KVLEN = false, SPLITKV = true, PAGED = false;
#define SAGE_ATTN_BODY_OF_KERNEL
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_OF_KERNEL
}

// the attention launch over (b, h, q-block, split) of a causal call; its merge is splitkv_merge_kernel<.., CAUSAL = true>
// (sage_attn_splitkv.hip), which derives the count of splits of a row's q-block as the workgroups above do
int launch_splitkv_causal_attn(const AttnCall& c, hipStream_t st) {
  return launch_4wave_kernel(c, st, c.p.nqb * c.p.Hq * c.p.B * c.p.num_splits, [](auto d, auto k, auto v, auto fp8) {
    return attn_i8_splitkv_causal_kernel<decltype(d)::value, decltype(k)::value, decltype(v)::value, decltype(fp8)::value>;
  });
}

}  // namespace sage
