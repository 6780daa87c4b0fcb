// Host-only probe of tests/test_kvlen.py: the status sage::attn_check (csrc/sage_attn.hip) gives per-batch key lengths
// combined with each form they are not built with.  The C ABI cannot express these combinations -- the _kvlen entry points
// have no list, mask, cu_seqlens or layout argument -- so the probe fills the argument block of the host layer itself.
// attn_check makes no HIP call and the addresses are never dereferenced.  Prints one "label status" line per case.
#include <cstdio>

#include "sage_entry.h"

int main() {
  using namespace sage;
  void* const fake = reinterpret_cast<void*>(1 << 20);
  const sage_tensor t{fake, 1 << 16, 1 << 12, 64};
  const int64_t mask_strides[4] = {0, 0, 333, 1};
  const sage_kv_layout layout{0, 0, 0, 0, 0};
  auto with_lens = [&] {
    AttnArgs a;
    a.q = a.k8 = a.v = a.o = &t;
    a.q_scale = a.k_scale = static_cast<const float*>(fake);
    a.B = 1; a.Hq = 2; a.Hk = 1; a.M = 200; a.N = 333; a.D = 64;
    a.qk_gran = SAGE_GRAN_PER_THREAD; a.blkq = 128; a.warpq = 32; a.sm_scale = 0.125f;
    a.key_lens = true; a.kv_lens = static_cast<const int32_t*>(fake);
    return a;
  };
  AttnCall c;
  AttnArgs a = with_lens();
  std::printf("alone %d\n", attn_check(c, a));
  a = with_lens();
  a.block_sparse = true; a.block_lists = static_cast<const int32_t*>(fake); a.block_lists_bytes = int64_t(1) << 40;
  std::printf("lists %d\n", attn_check(c, a));
  a = with_lens();
  a.mask = fake; a.mask_kind = 1; a.mask_strides = mask_strides;
  std::printf("mask %d\n", attn_check(c, a));
  a = with_lens();
  a.cu_q = a.cu_k = static_cast<const int*>(fake);
  std::printf("cu_seqlens %d\n", attn_check(c, a));
  a = with_lens();
  a.kvl = &layout;
  std::printf("layout %d\n", attn_check(c, a));
  a = with_lens();
  a.kv_lens = nullptr;
  std::printf("null %d\n", attn_check(c, a));
  a = with_lens();
  a.kv_lens = reinterpret_cast<const int32_t*>((1 << 20) + 2);
  std::printf("misaligned %d\n", attn_check(c, a));
  return 0;
}
