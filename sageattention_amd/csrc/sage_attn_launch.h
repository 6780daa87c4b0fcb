// The launch of a 4-wave attention kernel without attn_mask, written once for the block-sparse kernels (sage_attn.hip,
// sage_attn_pvskip.hip, sage_attn_sparse_kvlen.hip, sage_attn_sparse_kvlen_pvskip.hip) and the split-KV kernels
// (sage_attn_splitkv.hip, sage_attn_splitkv_causal.hip and their paged twins sage_attn_splitkv_paged.hip,
// sage_attn_splitkv_causal_paged.hip).  Each file instantiates its own kernel: it passes a generic callable
// that returns the kernel for (D, KTHREAD, V_BF16, PV_FP8), given as std::integral_constant / std::bool_constant values.
#pragma once
#include "sage_entry.h"

namespace sage {

// `grid` workgroups of 4 waves; the kernel's causal / sparse / ... flags are its own; fp8 V has no bf16 flavour
template <class KernelOf>
static int launch_4wave_kernel(const AttnCall& c, hipStream_t st, int grid, KernelOf kernel_of) {
  return by_dim(c.D, [&](auto d) {
    return by_flag(c.pv_fp8, [&](auto fp8) {
      constexpr int D = decltype(d)::value;
      constexpr bool PV_FP8 = decltype(fp8)::value;
      constexpr size_t smem = attn_lds_bytes(D, 4, PV_FP8);
      return by_flag(c.kthread, [&](auto k) {
        return by_flag(c.v_bf16, [&](auto v) {
          void (*kern)(const AttnParams) = kernel_of(d, k, std::bool_constant<!PV_FP8 && decltype(v)::value>{}, fp8);
          if (!allow_lds((const void*)kern, smem)) return (int)SAGE_ERR_LAUNCH;
          hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, c.p);
          return launch_status();
        });
      });
    });
  });
}

// slot count of a merge kernel (splitkv_merge_kernel, sage_attn_splitkv.hip; prefix_merge_kernel, sage_attn_prefix.hip) as a
// compile-time constant: the first of 2, 4, 8, 16 that holds S
template <class F>
static void by_slots(int count, F&& f) {
  if (count <= 2) f(std::integral_constant<int, 2>{});
  else if (count <= 4) f(std::integral_constant<int, 4>{});
  else if (count <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

}  // namespace sage
