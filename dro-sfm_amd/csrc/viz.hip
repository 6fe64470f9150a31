// Depth inference outputs: the per-image percentile that normalises an inverse
// depth map, the colour-map lookup with the RGB-over-depth panel, and the
// scanlines of a 16-bit depth PNG.
//
// Replaces, of the reference:
//   viz_inv_depth   dro_sfm/utils/depth.py:65-99   .cpu(), np.percentile (a full
//                                                  sort), the matplotlib lookup
//   write_depth     dro_sfm/utils/depth.py:34-62   (depth * 256).int() -> PIL mode I
//                                                  -> 16-bit PNG (the scanlines;
//                                                  deflate stays on the host)
//   the panel       scripts/infer.py:160-181       frame * 255 over colour * 255,
//                                                  written by imwrite
//
// percentile: one 1024-thread block per row does every pass of a radix select
// in one launch -- four 8-bit digit passes for the order statistic a[lo], and
// one more pass for its successor a[hi] when a[lo]'s ties do not already
// cover it.  Only integer counts decide, so the result does not depend on the
// order in which threads arrive: bitwise deterministic.  A 192x640 map is
// 480 KB: the passes after the first read it from L2.  Measured (DESIGN.md
// §11): 94 us a call at 192x640 for B = 1 and for B = 4, about 19 us a pass
// whatever the number of loads in flight; fewer instructions per value is
// what made it faster.
#include <hip/hip_runtime.h>

#include <math.h>

#include "dro_common.hpp"

namespace dro {

constexpr int kPctThreads = 1024;
constexpr int kPctWaves = kPctThreads / kWave;
constexpr int kPctUnroll = 8;          // independent loads in flight per thread
constexpr int kVizThreads = 256;

// IEEE bits -> a key whose unsigned order is the order of the values
// (negatives reversed below the positives; -0.0 just below +0.0)
__device__ __forceinline__ unsigned order_key(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_value(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__global__ __launch_bounds__(kPctThreads) void percentile_kernel(const float* __restrict__ values, long long n,
                                                                 double q, int filter_zeros,
                                                                 float* __restrict__ out) {
  __shared__ unsigned h[kPctWaves][256];
  __shared__ unsigned hs[256];
  __shared__ unsigned s_prefix, s_k, s_le, s_m, s_min;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
  const float* __restrict__ row = values + (size_t)blockIdx.x * (size_t)n;
  unsigned prefix = 0u, k = 0u, m = 0u;
  const unsigned un = (unsigned)n, step = kPctThreads * kPctUnroll;   // n < 2^31: indices fit 32 bits
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
    for (int i = tid; i < kPctWaves * 256; i += kPctThreads) (&h[0][0])[i] = 0u;
    __syncthreads();
    // A thread counts runs: the values it meets in a row of a depth map mostly
    // share their upper digits, so it adds to the wave's histogram only when
    // the bin changes (one atomic per value at worst, on the low digits).
    unsigned run_bin = 0u, run = 0u;
    for (unsigned base = 0; base < un; base += step) {
      float x[kPctUnroll];
#pragma unroll
      for (int j = 0; j < kPctUnroll; ++j) {
        const unsigned i = base + j * kPctThreads + tid;
        x[j] = i < un ? row[i] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < kPctUnroll; ++j) {
        const unsigned i = base + j * kPctThreads + tid;
        const unsigned key = order_key(x[j]);
        const unsigned bin = (key >> shift) & 255u;
        if (i < un && (!filter_zeros || x[j] > 0.f) && (key & himask) == prefix) {
          if (bin != run_bin) {
            if (run) atomicAdd(&h[wid][run_bin], run);
            run_bin = bin;
            run = 0u;
          }
          ++run;
        }
      }
    }
    if (run) atomicAdd(&h[wid][run_bin], run);
    __syncthreads();
    if (tid < 256) {
      unsigned s = 0u;
      for (int w = 0; w < kPctWaves; ++w) s += h[w][tid];
      hs[tid] = s;
    }
    __syncthreads();
    if (wid == 0) {
      // lane l owns bins 4l..4l+3; inclusive scan of the lanes' sums
      unsigned c[4], own = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[j] = hs[4 * lane + j];
        own += c[j];
      }
      unsigned incl = own;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += up;
      }
      unsigned kk = k;
      if (pass == 0) {
        const unsigned total = __shfl(incl, kWave - 1, kWave);
        // lo = floor((m - 1) q / 100), at most m - 1
        unsigned lo = 0u;
        if (total > 0u) {
          const double v = (double)(total - 1u) * q / 100.0;
          lo = (unsigned)fmin(floor(v), (double)(total - 1u));
        }
        kk = lo;
        if (lane == 0) s_m = total;
      }
      unsigned below = incl - own;
      if (kk >= below && kk < incl) {      // one lane, when the row is not empty
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (kk >= below && kk < below + c[j]) {
            s_prefix = prefix | ((unsigned)(4 * lane + j) << shift);
            s_k = kk - below;
            s_le = c[j] - (kk - below);    // keys in the chosen bin from rank kk on
          }
          below += c[j];
        }
      }
    }
    __syncthreads();
    if (pass == 0) {
      m = s_m;
      if (m == 0u) {                       // block-uniform
        if (tid == 0) out[blockIdx.x] = __uint_as_float(0x7FC00000u);
        return;
      }
    }
    prefix = s_prefix;
    k = s_k;
  }
  // prefix is a[lo]'s key; s_le of the last pass counts a[lo]'s ties from rank lo on
  const double v = (double)(m - 1u) * q / 100.0;
  const double lo_d = fmin(floor(v), (double)(m - 1u));
  const unsigned lo = (unsigned)lo_d;
  const bool need_next = lo + 1u < m && s_le < 2u;   // a[hi] is a larger value
  unsigned hi_key = prefix;
  if (need_next) {                                   // block-uniform
    if (tid == 0) s_min = 0xFFFFFFFFu;
    __syncthreads();
    unsigned best = 0xFFFFFFFFu;
    for (unsigned base = 0; base < un; base += step) {
      float x[kPctUnroll];
#pragma unroll
      for (int j = 0; j < kPctUnroll; ++j) {
        const unsigned i = base + j * kPctThreads + tid;
        x[j] = i < un ? row[i] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < kPctUnroll; ++j) {
        const unsigned i = base + j * kPctThreads + tid;
        const unsigned key = order_key(x[j]);
        if (i < un && (!filter_zeros || x[j] > 0.f) && key > prefix) best = min(best, key);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, kWave));
    if (lane == 0) atomicMin(&s_min, best);
    __syncthreads();
    hi_key = s_min;
  }
  if (tid == 0) {
    const double a = (double)key_value(prefix), b = (double)key_value(hi_key);
    out[blockIdx.x] = (float)(a + (b - a) * (v - lo_d));
  }
}

// ---------------------------------------------------------------- colorize
__device__ __forceinline__ unsigned char to_byte(float v) {   // rint(255 v) saturated; NaN -> 0
  return (unsigned char)fminf(fmaxf(rintf(255.f * v), 0.f), 255.f);
}

__global__ __launch_bounds__(kVizThreads) void colorize_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ norm,
                                                               const float* __restrict__ lut,
                                                               const float* __restrict__ rgb, int HW,
                                                               float* __restrict__ color,
                                                               unsigned char* __restrict__ panel) {
  __shared__ float table[256 * 3];
  for (int i = threadIdx.x; i < 256 * 3; i += kVizThreads) table[i] = lut[i];
  __syncthreads();
  const int p = blockIdx.x * kVizThreads + threadIdx.x;   // H*W < 2^31 - 256 (checked by the caller)
  if (p >= HW) return;
  const int b = blockIdx.y;
  const size_t px = (size_t)b * HW + p;
  // matplotlib, 256 entries, floats in: clip to [0, 1], times 256, truncated,
  // 256 itself taken down to 255; NaN is "bad": (0, 0, 0)
  const float t = x[px] / (norm[b] + 1e-6f);
  float c[3] = {0.f, 0.f, 0.f};
  if (t == t) {
    const int k = min((int)(fminf(fmaxf(t, 0.f), 1.f) * 256.f), 255);
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = table[3 * k + j];
  }
  if (color) {
#pragma unroll
    for (int j = 0; j < 3; ++j) color[px * 3 + j] = c[j];
  }
  if (panel) {
    unsigned char* top = panel + ((size_t)b * 2 * HW + p) * 3;
    unsigned char* bottom = top + (size_t)HW * 3;
    const float* frame = rgb + (size_t)b * 3 * HW + p;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      top[j] = to_byte(frame[(size_t)j * HW]);
      bottom[j] = to_byte(c[j]);
    }
  }
}

// ---------------------------------------------------------------- depth_png16_rows
__global__ __launch_bounds__(kVizThreads) void depth_png16_rows_kernel(const float* __restrict__ depth, int HW,
                                                                       int W, unsigned char* __restrict__ rows) {
  const int p = blockIdx.x * kVizThreads + threadIdx.x;   // H*W < 2^31 - 256 (checked by the caller)
  if (p >= HW) return;
  const int y = p / W, xcol = p - y * W;
  const int H = HW / W;
  const float v = depth[(size_t)blockIdx.y * HW + p] * 256.f;
  // trunc, then Pillow's clamp of a mode-I image saved as 16-bit; NaN -> 0
  const unsigned u = !(v > 0.f) ? 0u : (v >= 65535.f ? 65535u : (unsigned)v);
  unsigned char* line = rows + ((size_t)blockIdx.y * H + y) * (size_t)(1 + 2 * (size_t)W);
  if (xcol == 0) line[0] = 0;                              // filter type None
  line[1 + 2 * xcol] = (unsigned char)(u >> 8);
  line[2 + 2 * xcol] = (unsigned char)(u & 255u);
}

static bool bad_image(int B, int H, int W) {
  return B < 1 || B > 65535 || H < 1 || W < 1 || (long long)H * W >= (1LL << 31) - kVizThreads;
}

}  // namespace dro

using namespace dro;

extern "C" int dro_percentile(const float* values, int B, long long n, double q, int filter_zeros, float* out,
                              void* stream) {
  if (!values || !out) {
    set_error("percentile: NULL pointer");
    return DRO_E_NULL;
  }
  if (B < 1 || B > 65535 || n < 1 || n >= (1LL << 31)) {
    set_error("percentile: sizes out of range (B 1..65535, 1 <= n < 2^31)");
    return DRO_E_SHAPE;
  }
  if (!(q >= 0.0 && q <= 100.0)) {
    set_error("percentile: q outside [0, 100] or NaN");
    return DRO_E_MODE;
  }
  hipLaunchKernelGGL(percentile_kernel, dim3(B), dim3(kPctThreads), 0, (hipStream_t)stream, values, n, q,
                     filter_zeros ? 1 : 0, out);
  return launch_status("percentile_kernel launch failed");
}

extern "C" int dro_colorize(const float* x, const float* norm, const float* lut, const float* rgb, int B, int H,
                            int W, float* color, unsigned char* panel, void* stream) {
  if (!x || !norm || !lut || (!color && !panel) || (panel && !rgb)) {
    set_error("colorize: NULL pointer (x, norm, lut; color or panel; rgb with panel)");
    return DRO_E_NULL;
  }
  if (bad_image(B, H, W)) {
    set_error("colorize: sizes out of range (B 1..65535, H, W >= 1, H*W < 2^31)");
    return DRO_E_SHAPE;
  }
  hipLaunchKernelGGL(colorize_kernel, dim3((H * W + kVizThreads - 1) / kVizThreads, B), dim3(kVizThreads), 0,
                     (hipStream_t)stream, x, norm, lut, rgb, H * W, color, panel);
  return launch_status("colorize_kernel launch failed");
}

extern "C" int dro_depth_png16_rows(const float* depth, int B, int H, int W, unsigned char* rows, void* stream) {
  if (!depth || !rows) {
    set_error("depth_png16_rows: NULL pointer");
    return DRO_E_NULL;
  }
  if (bad_image(B, H, W)) {
    set_error("depth_png16_rows: sizes out of range (B 1..65535, H, W >= 1, H*W < 2^31)");
    return DRO_E_SHAPE;
  }
  hipLaunchKernelGGL(depth_png16_rows_kernel, dim3((H * W + kVizThreads - 1) / kVizThreads, B), dim3(kVizThreads),
                     0, (hipStream_t)stream, depth, H * W, W, rows);
  return launch_status("depth_png16_rows_kernel launch failed");
}
