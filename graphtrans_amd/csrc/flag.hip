// flag.hip — the ascent step of FLAG adversarial training (Kong et al., "Robust Optimization as Data Augmentation for Large-scale
// Graphs"): between two of the m forward / backward passes of one batch the perturbation moves one step along the sign of its
// gradient and the gradient is cleared,
//   perturb <- perturb + step * sign(perturb.grad);  perturb.grad <- 0
// which the reference's trainer writes as detach, sign, mul, add and a zero fill (trainers/flag_trainer.py:41-43: five launches and
// three [N][D] temporaries).  Here it is one pass: one 16-byte load of each operand, one 16-byte store of each.
#include "gt_common.h"

namespace {

constexpr int FT = 256;
constexpr int64_t FLAG_MAX_BLOCKS = 2048;   // 8 blocks per CU; longer vectors take more trips of the stride loop

// torch.sign is (0 < g) - (g < 0): 1 / -1 by the comparisons and +0 where neither holds -- a zero of either sign, and NaN too (a NaN
// gradient element leaves its perturbation element where it is, in torch and here)
__device__ __forceinline__ float flag_sign(float g) { return g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f); }

__global__ void __launch_bounds__(FT) k_flag_ascent(float* __restrict__ perturb, float* __restrict__ grad, int64_t n4, float step) {
  for (int64_t i = (int64_t)blockIdx.x * FT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * FT) {
    const float4 g = *reinterpret_cast<const float4*>(grad + i * 4);
    float4 p = *reinterpret_cast<const float4*>(perturb + i * 4);
    // step * (+-1) is exact, so a contracted multiply-add rounds like torch's separate mul and add
    p.x += step * flag_sign(g.x);
    p.y += step * flag_sign(g.y);
    p.z += step * flag_sign(g.z);
    p.w += step * flag_sign(g.w);
    *reinterpret_cast<float4*>(perturb + i * 4) = p;
    *reinterpret_cast<float4*>(grad + i * 4) = gt_zero4();
  }
}

}  // namespace

extern "C" int gt_flag_ascent(float* perturb, float* grad, int64_t n, float step, gt_stream_t stream_) {
  if (n < 0 || n % 4) { gt_set_error("gt_flag_ascent: the element count must be a multiple of 4"); return GT_ERR_UNSUPPORTED; }
  if (n == 0) return GT_OK;
  GT_CHECK_ARG(perturb && grad && perturb != grad, "null or aliased buffer");
  GT_CHECK_ARG(!(((uintptr_t)perturb | (uintptr_t)grad) & 15), "16-byte aligned buffers");
  const int64_t n4 = n / 4, blocks = gt_cdiv(n4, FT);
  hipLaunchKernelGGL(k_flag_ascent, dim3((unsigned)(blocks < FLAG_MAX_BLOCKS ? blocks : FLAG_MAX_BLOCKS)), dim3(FT), 0, (hipStream_t)stream_,
                     perturb, grad, n4, step);
  GT_CHECK_LAUNCH();
  return GT_OK;
}
