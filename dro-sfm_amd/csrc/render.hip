// Point-cloud rendering: the cumulative cloud of a reconstructed sequence drawn
// as square splats through a software z-buffer, all views in one call.
//
// Stands in for, of the reference's scripts/vis.py:
//   create_pointcloud_actor + vtkTimerCallback.execute  :259-360  a vtk point
//                                 actor of size 5 on black, rendered through
//                                 OpenGL once per frame and read back
// There is no vtk or OpenGL on a headless MI355X server; the picture here is a
// deterministic function of the cloud, the camera and the point size.
//
// Three launches on the caller's stream, nothing allocated here, capturable:
//   fill     the z-buffer [V, H+2m, W+2m] of 64-bit keys with all ones
//            (m = point_size / 2: the margin that lets a centre just off the
//            image paint the pixels its square overlaps)
//   splat    one thread per (point, view): camera point R p + t, pinhole
//            projection, rintf to the pixel centre (half to even), one
//            atomicMin of (float_bits(z) << 32) | point_index.  z > 0 makes the
//            float bits monotone, and the minimum of a set does not depend on
//            the order of arrival: the result is bitwise deterministic and
//            equal depths resolve to the lowest point index.
//   resolve  one thread per output pixel: the minimum key over the s x s
//            window of centres whose square covers the pixel (the minimum over
//            a union of squares, with one atomic per point instead of s^2),
//            then colour, depth and index of the winner.
// Everything is fp32 and this object is built with -ffp-contract=off: every
// product and sum below is rounded on its own, in the order written, so
// tests/render_oracle.py can restate it operation by operation.
#include <hip/hip_runtime.h>

#include "dro_common.hpp"

namespace dro {

constexpr int kRenderThreads = 256;
constexpr int kRenderMaxPointSize = 15;
constexpr int kRenderMaxFillBlocks = 1 << 16;
constexpr unsigned long long kRenderEmpty = ~0ull;
constexpr int kRenderRejected = -1;   // rec_pixel of a (view, point) pair that wrote no key

__global__ __launch_bounds__(kRenderThreads) void render_fill_kernel(unsigned long long* __restrict__ zbuf,
                                                                     size_t total) {
  const size_t stride = (size_t)gridDim.x * kRenderThreads;
  for (size_t i = (size_t)blockIdx.x * kRenderThreads + threadIdx.x; i < total; i += stride) zbuf[i] = kRenderEmpty;
}

// kEarlySkip: read the pixel's current key first (relaxed, agent scope) and
// leave the atomic out when this point cannot win.  Keys only ever decrease,
// so a stale read costs an atomic that was not needed, never a wrong skip.
// Measured SLOWER than sending every atomic (1.55 against 1.26 ms and 0.50
// against 0.40 ms per call, profiles/render_throughput.txt): the load is a
// second round trip to L2 for every pair, while an atomic whose result is not
// used need not be waited for (supposed, not profiled).  Off by default; kept
// for tools/render_throughput.py.
template <bool kEarlySkip>
__global__ __launch_bounds__(kRenderThreads) void render_splat_kernel(
    const float* __restrict__ xyz, int n, const float* __restrict__ K, const float* __restrict__ world2cam,
    const int* __restrict__ limit, int H, int W, int margin, float near, unsigned long long* __restrict__ zbuf,
    int* __restrict__ rec_pixel, unsigned int* __restrict__ rec_zbits) {
  const long long gi = (long long)blockIdx.x * kRenderThreads + threadIdx.x;
  if (gi >= n) return;
  const int i = (int)gi;
  const int v = blockIdx.y;
  const int lim = limit ? limit[v] : n;
  int pixel = kRenderRejected;
  unsigned int zbits = 0u;
  if (i < lim) {
    const float* Kv = K + (size_t)v * 9;
    const float fx = Kv[0], fy = Kv[4], cx = Kv[2], cy = Kv[5];
    float R[9], t[3];
    load_pose(world2cam + (size_t)v * 16, DRO_POSE_MATRIX, R, t);
    const float* p = xyz + (size_t)i * 3;
    const float p0 = p[0], p1 = p[1], p2 = p[2];
    const float x = R[0] * p0 + R[1] * p1 + R[2] * p2 + t[0];
    const float y = R[3] * p0 + R[4] * p1 + R[5] * p2 + t[1];
    const float z = R[6] * p0 + R[7] * p1 + R[8] * p2 + t[2];
    const bool finite = fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;   // false on NaN
    if (finite && z >= near) {
      const float u = fx * x / z + cx, w = fy * y / z + cy;
      // the range test is made in float, before any integer conversion (|u|
      // may be huge, infinite or NaN: then outside)
      const float ur = rintf(u), wr = rintf(w);
      const float fm = (float)margin;
      if (ur >= -fm && ur <= (float)(W - 1) + fm && wr >= -fm && wr <= (float)(H - 1) + fm) {
        const int Wp = W + 2 * margin;
        pixel = ((int)wr + margin) * Wp + ((int)ur + margin);
        zbits = __float_as_uint(z);
        const unsigned long long key = ((unsigned long long)zbits << 32) | (unsigned int)i;
        unsigned long long* cell = zbuf + (size_t)v * (H + 2 * margin) * Wp + pixel;
        bool send = true;
        if (kEarlySkip) send = key < __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (send) atomicMin(cell, key);
      }
    }
  }
  if (rec_pixel) rec_pixel[(size_t)v * n + i] = pixel;
  if (rec_zbits) rec_zbits[(size_t)v * n + i] = zbits;
}

__device__ __forceinline__ unsigned char render_byte(float v) {   // rint(255 v) saturated; NaN -> 0
  return (unsigned char)fminf(fmaxf(rintf(255.f * v), 0.f), 255.f);
}

__global__ __launch_bounds__(kRenderThreads) void render_resolve_kernel(
    const unsigned long long* __restrict__ zbuf, const float* __restrict__ rgb, int H, int W, int point_size,
    unsigned int background, unsigned char* __restrict__ image, float* __restrict__ depth,
    int* __restrict__ index) {
  const int p = blockIdx.x * kRenderThreads + threadIdx.x;   // H*W <= 2^30 (checked by the caller)
  if (p >= H * W) return;
  const int v = blockIdx.y;
  const int margin = point_size / 2;
  const int Wp = W + 2 * margin;
  const int y = p / W, x = p - y * W;
  // centres c with c - s/2 <= pixel <= c + (s-1)/2, in padded coordinates
  const int lo = -((point_size - 1) / 2), hi = point_size / 2;
  const unsigned long long* view = zbuf + (size_t)v * (H + 2 * margin) * Wp;
  unsigned long long best = kRenderEmpty;
  for (int dy = lo; dy <= hi; ++dy) {
    const unsigned long long* row = view + (size_t)(y + margin + dy) * Wp + (x + margin);
    for (int dx = lo; dx <= hi; ++dx) {
      const unsigned long long k = row[dx];
      best = k < best ? k : best;
    }
  }
  const size_t o = (size_t)v * H * W + p;
  unsigned char* px = image + o * 3;
  if (best == kRenderEmpty) {
    px[0] = (unsigned char)(background & 255u);
    px[1] = (unsigned char)((background >> 8) & 255u);
    px[2] = (unsigned char)((background >> 16) & 255u);
    if (depth) depth[o] = 0.f;
    if (index) index[o] = -1;
    return;
  }
  const unsigned int i = (unsigned int)(best & 0xffffffffull);
  const float* c = rgb + (size_t)i * 3;
  px[0] = render_byte(c[0]);
  px[1] = render_byte(c[1]);
  px[2] = render_byte(c[2]);
  if (depth) depth[o] = __uint_as_float((unsigned int)(best >> 32));
  if (index) index[o] = (int)i;
}

static bool bad_render(int V, int H, int W, int s) {
  // H, W <= 32768: the padded map stays below 2^31 cells and every pixel
  // coordinate is exact in float (the splat's range test)
  return V < 1 || V > 65535 || H < 1 || W < 1 || H > 32768 || W > 32768 || s < 1 || s > kRenderMaxPointSize;
}

}  // namespace dro

using namespace dro;

extern "C" size_t dro_render_points_workspace_bytes(int V, int H, int W, int point_size) {
  if (bad_render(V, H, W, point_size)) return 0;
  const int m = point_size / 2;
  return (size_t)V * (size_t)(H + 2 * m) * (size_t)(W + 2 * m) * sizeof(unsigned long long);
}

extern "C" int dro_render_points(const float* xyz, const float* rgb, long long n, const float* K,
                                 const float* world2cam, const int* limit, int V, int H, int W, int point_size,
                                 float near, unsigned int background, unsigned char* image, float* depth,
                                 int* index, int* rec_pixel, unsigned int* rec_zbits, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if ((n > 0 && (!xyz || !rgb)) || !K || !world2cam || !image || !workspace) {
    set_error("render_points: NULL pointer");
    return DRO_E_NULL;
  }
  if (bad_render(V, H, W, point_size) || n < 0 || n > 2147483647LL) {
    set_error("render_points: sizes out of range (V 1..65535, H, W 1..32768, point_size 1..15, "
              "0 <= n <= 2^31 - 1)");
    return DRO_E_SHAPE;
  }
  const size_t need = dro_render_points_workspace_bytes(V, H, W, point_size);
  if (workspace_bytes < need) {
    set_error("render_points: workspace smaller than dro_render_points_workspace_bytes");
    return DRO_E_SHAPE;
  }
  if (!(near > 0.f) || !(near < INFINITY)) {
    set_error("render_points: near must be positive and finite (z > 0 makes the depth keys monotone)");
    return DRO_E_MODE;
  }
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* zbuf = (unsigned long long*)workspace;
  const size_t cells = need / sizeof(unsigned long long);
  const size_t fill_blocks = (cells + kRenderThreads - 1) / kRenderThreads;
  hipLaunchKernelGGL(render_fill_kernel,
                     dim3((unsigned)(fill_blocks < (size_t)kRenderMaxFillBlocks ? fill_blocks : kRenderMaxFillBlocks)),
                     dim3(kRenderThreads), 0, s, zbuf, cells);
  int st = launch_status("render_fill_kernel launch failed");
  if (st) return st;
  const int m = point_size / 2;
  if (n > 0) {
    const dim3 grid((unsigned)((n + kRenderThreads - 1) / kRenderThreads), V);
    // DRO_RENDER_EARLY_SKIP=1: the other splat variant (A/B measurements)
    if (env_int("DRO_RENDER_EARLY_SKIP", 0)) {
      hipLaunchKernelGGL(render_splat_kernel<true>, grid, dim3(kRenderThreads), 0, s, xyz, (int)n, K, world2cam,
                         limit, H, W, m, near, zbuf, rec_pixel, rec_zbits);
    } else {
      hipLaunchKernelGGL(render_splat_kernel<false>, grid, dim3(kRenderThreads), 0, s, xyz, (int)n, K, world2cam,
                         limit, H, W, m, near, zbuf, rec_pixel, rec_zbits);
    }
    st = launch_status("render_splat_kernel launch failed");
    if (st) return st;
  }
  hipLaunchKernelGGL(render_resolve_kernel, dim3((H * W + kRenderThreads - 1) / kRenderThreads, V),
                     dim3(kRenderThreads), 0, s, zbuf, rgb, H, W, point_size, background, image, depth, index);
  return launch_status("render_resolve_kernel launch failed");
}
