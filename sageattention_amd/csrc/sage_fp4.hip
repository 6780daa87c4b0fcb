// The stand-alone MXFP4 V quantizer (the rule: include/sageattn_hip_fp4.h; the unit body: sage_fp4_kernels.h).  One launch of
// (units, H, B) workgroups, one pass over V: 2 bytes read and 0.53 written per element.  A workgroup whose unit lies at or
// beyond the batch's last tile returns before any barrier and writes nothing.
#include "sage_fp4_kernels.h"
#include "../../include/sageattn_hip_fp4.h"

namespace sage {

template <int D, bool BF16>
__global__ __launch_bounds__(256) void v_quant_mxfp4_kernel(const uint16_t* __restrict__ v, const int64_t sb, const int64_t sh,
                                                            const int64_t sn, const int N, const V4Image o,
                                                            const int32_t* __restrict__ kv_lens) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[V4QuantGeom<D>::LDS];
  const int unit = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int len = kv_lens ? min(max(kv_lens[b], 0), N) : N;
  if (unit * VQuantGeom<D>::BLKS * 64 >= len) return;
  v4_quant_unit<D, BF16>(v, sb, sh, sn, len, o, unit, 0, h, b, lds);
}

}  // namespace sage

using namespace sage;

extern "C" int sage_quant_v_mxfp4(const sage_tensor* v, int dtype, int B, int H, int N, int D, const sage_tensor* img,
                                  uint8_t* scale, const int32_t* kv_lens, sage_stream_t stream) {
  if (!tensor_ok(v, 8) || !tensor_ok(img, 16) || !scale || !aligned16(scale) || ((uintptr_t)kv_lens & 3)) return SAGE_ERR_INVALID_ARGUMENT;
  if (B <= 0 || H <= 0 || N <= 0) return SAGE_ERR_INVALID_ARGUMENT;
  if (const int s = dim_dtype_status(D, dtype)) return s;
  const int T = (N + 63) / 64;
  V4Image o;
  o.img = (uint8_t*)img->data; o.ob = img->stride_b; o.oh = img->stride_h; o.od = img->stride_n;
  o.scale = scale; o.sh = (int64_t)T * 2 * D; o.sb = o.sh * H;
  launch_begin();
  by_dim(D, [&](auto d) {
    by_flag(dtype == SAGE_BF16, [&](auto bf) {
      constexpr int DD = decltype(d)::value;
      const int units = (T + VQuantGeom<DD>::BLKS - 1) / VQuantGeom<DD>::BLKS;
      hipLaunchKernelGGL((v_quant_mxfp4_kernel<DD, decltype(bf)::value>), dim3(units, H, B), dim3(256), 0, (hipStream_t)stream,
                         (const uint16_t*)v->data, v->stride_b, v->stride_h, v->stride_n, N, o, kv_lens);
    });
  });
  return launch_status();
}
