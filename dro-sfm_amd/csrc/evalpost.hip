// Test-time left-right flip post-processing of the evaluation step.
//
// Replaces post_process_inv_depth (dro_sfm/utils/depth.py:202-256 of the
// reference) and the two inv2depth calls around it in
// ModelWrapper.evaluate_depth (dro_sfm/models/model_wrapper.py:361-371):
// flip_lr of the flipped pass, fuse (mean / max / min), the linspace ramp
// masks of the two image borders, the blend, and both depth maps -- ~15 ATen
// launches there, one launch here.  Per pixel, in the reference's operation
// order with explicit roundings (no contraction):
//   a = inv[b,y,x], bh = inv_flipped[b,y,W-1-x], f = fuse(a, bh)
//   xs = linspace(0,1,W)[x], mask = 1 - clamp(20 (xs - 0.05), 0, 1),
//   mask_hat = the same at column W-1-x
//   inv_pp = (mask_hat a + mask bh) + ((1 - mask) - mask_hat) f
//   depth = inv2depth(a), depth_pp = inv2depth(inv_pp)
// Roofline: HBM bound.  Algorithmic bytes per pixel: 8 read (inv,
// inv_flipped) + 12 written (inv_pp, depth, depth_pp).  No LDS: the mirrored
// read stays inside the cache lines of the same image row.
#include <hip/hip_runtime.h>

#include "dro_common.hpp"

namespace dro {

constexpr int kPostThreads = 256;

// torch.linspace(0, 1, W)[x] as ATen's kernels form it: step = 1 / (W - 1),
// the lower half counted up from 0, the upper half down from 1
__device__ __forceinline__ float post_linspace(int x, int W, float step) {
  return x < W / 2 ? __fmul_rn(step, (float)x) : __fadd_rn(1.f, -__fmul_rn(step, (float)(W - 1 - x)));
}

// 1 - clamp(20 (xs - 0.05), 0, 1)
__device__ __forceinline__ float post_mask(float xs) {
  const float r = __fmul_rn(20.f, __fadd_rn(xs, -0.05f));
  return __fadd_rn(1.f, -fminf(fmaxf(r, 0.f), 1.f));
}

// inv2depth (utils/depth.py:102-121): 1 / clamp(v, 1e-6), 0 where v <= 0
__device__ __forceinline__ float post_inv2depth(float v) {
  return v <= 0.f ? 0.f : __fdiv_rn(1.f, fmaxf(v, 1e-6f));
}

__global__ __launch_bounds__(kPostThreads) void post_process_inv_depth_kernel(
    const float* __restrict__ inv, const float* __restrict__ inv_flipped, int HW, int W, int method, float step,
    float* __restrict__ inv_pp, float* __restrict__ depth, float* __restrict__ depth_pp) {
  const int p = blockIdx.x * kPostThreads + threadIdx.x;   // HW < 2^31 - 256 (checked by the caller)
  if (p >= HW) return;
  const size_t base = (size_t)blockIdx.y * HW;
  const int x = p % W, xm = W - 1 - x;
  const float a = inv[base + p];
  const float bh = inv_flipped[base + (p - x) + xm];
  float f;
  if (method == 0) f = __fmul_rn(0.5f, __fadd_rn(a, bh));
  else if (method == 1) f = fmaxf(a, bh);
  else f = fminf(a, bh);
  const float mask = post_mask(post_linspace(x, W, step));
  const float mask_hat = post_mask(post_linspace(xm, W, step));
  const float edge = __fadd_rn(__fmul_rn(mask_hat, a), __fmul_rn(mask, bh));
  const float mid = __fmul_rn(__fadd_rn(__fadd_rn(1.f, -mask), -mask_hat), f);
  const float pp = __fadd_rn(edge, mid);
  inv_pp[base + p] = pp;
  depth[base + p] = post_inv2depth(a);
  depth_pp[base + p] = post_inv2depth(pp);
}

}  // namespace dro

using namespace dro;

extern "C" int dro_post_process_inv_depth(const float* inv, const float* inv_flipped, int B, int H, int W,
                                          int method, float* inv_pp, float* depth, float* depth_pp,
                                          void* stream) {
  if (!inv || !inv_flipped || !inv_pp || !depth || !depth_pp) {
    set_error("post_process_inv_depth: NULL pointer");
    return DRO_E_NULL;
  }
  if (B < 1 || H < 1 || W < 2 || B > 65535 || (long long)H * W >= (1LL << 31) - kPostThreads) {
    set_error("post_process_inv_depth: sizes out of range (B 1..65535, H >= 1, W >= 2, H*W < 2^31)");
    return DRO_E_SHAPE;
  }
  if (method < 0 || method > 2) {
    set_error("post_process_inv_depth: unknown method (0 mean, 1 max, 2 min)");
    return DRO_E_MODE;
  }
  const int HW = H * W;
  const float step = 1.f / (float)(W - 1);
  hipLaunchKernelGGL(post_process_inv_depth_kernel, dim3((HW + kPostThreads - 1) / kPostThreads, B),
                     dim3(kPostThreads), 0, (hipStream_t)stream, inv, inv_flipped, HW, W, method, step, inv_pp,
                     depth, depth_pp);
  return launch_status("post_process_inv_depth_kernel launch failed");
}
