// Sequence reconstruction after the network: depth cleaning, multi-view
// geometric consistency filter + depth fusion, back-projection to a packed
// world-space point cloud.
//
// Replaces, of the reference's scripts/infer_video.py:
//   depth_clean         :647-657  pad, squared forward differences, two
//                                 thresholds, two corner crops
//   depth_fusion        :254-369  reproject_with_depth_batch,
//                                 check_geometric_consistency_batch and the
//                                 sums of gemo_filter_fusion: ~70 ATen launches
//                                 per source view there (two torch.inverse and a
//                                 grid_sample among them), one launch for all
//                                 views here
//   backproject_points  :674-682  meshgrid, inv(K), the camera->world transform,
//                                 plus the compaction of the valid pixels
// Everything is fp32 and this object is built with -ffp-contract=off: every
// product and sum below is rounded on its own, in the order written, so the
// Python restatements can follow it operation by operation.
//
// Conventions: K is read as a pinhole (fx, fy, cx, cy); extrinsics are rigid
// world->camera [R | t] (row-major 4x4, the last row is not read); the rigid
// inverse [R^T | -R^T t] is formed in the kernel.
// Roofline: all three are HBM bound.  depth_fusion moves (8 + 4 S + 1) bytes
// per reference pixel (depth in, fused out, S gathered source depths, the
// count); the gathers stay within a few rows of the thread's own (nearby
// cameras), so they hit the lines the neighbouring threads pull in.
#include <hip/hip_runtime.h>

#include "dro_common.hpp"

namespace dro {

constexpr int kReconThreads = 256;
constexpr int kFusionMaxViews = 8;
constexpr int kPackRounds = 4;                                 // pixels per thread of the packing kernels
constexpr int kPackTile = kReconThreads * kPackRounds;         // pixels per block
constexpr int kPackWaves = kReconThreads / kWave;
// the recorded source pixel of a sample that fell outside the map: pack_cell
// clamps both coordinates to [-32767, 32766], so a y of 32767 never occurs
constexpr int kFusionOutside = -2;

// ---------------------------------------------------------------- depth_clean
__global__ __launch_bounds__(kReconThreads) void depth_clean_kernel(
    const float* __restrict__ depth, int H, int W, float grad_max, float depth_max, int crop_h, int crop_w,
    float* __restrict__ out) {
  const int p = blockIdx.x * kReconThreads + threadIdx.x;   // H*W < 2^31 - 256 (checked by the caller)
  if (p >= H * W) return;
  const size_t base = (size_t)blockIdx.y * H * W;
  const int y = p / W, x = p - y * W;
  const float d = depth[base + p];
  const float below = y + 1 < H ? depth[base + p + W] : 0.f;
  const float right = x + 1 < W ? depth[base + p + 1] : 0.f;
  const float gy = below - d, gx = right - d;
  const float g = gy * gy + gx * gx;
  const bool crop = crop_h > 0 && crop_w > 0 &&
                    ((y < crop_h && x < crop_w) || (y >= H - crop_h && x >= W - crop_w));
  out[base + p] = (g > grad_max || d > depth_max || crop) ? 0.f : d;
}

// ---------------------------------------------------------------- depth_fusion
// R [9], t [3] of the rigid transform A * B^-1 for world->camera A and B
__device__ __forceinline__ void relative_pose(const float* __restrict__ A, const float* __restrict__ B, float* R,
                                              float* t) {
  float Ra[9], Rb[9], ta[3], tb[3];
  load_pose(A, DRO_POSE_MATRIX, Ra, ta);
  load_pose(B, DRO_POSE_MATRIX, Rb, tb);
  // B^-1 = [Rb^T | -Rb^T tb]
  float RbT[9], tbi[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) RbT[3 * i + j] = Rb[3 * j + i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) tbi[i] = -(RbT[3 * i] * tb[0] + RbT[3 * i + 1] * tb[1] + RbT[3 * i + 2] * tb[2]);
  float Rm[9];
  mat3_mul(Ra, RbT, Rm);
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = Rm[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = Ra[3 * i] * tbi[0] + Ra[3 * i + 1] * tbi[1] + Ra[3 * i + 2] * tbi[2] + ta[i];
}

// pixel (u, v) at depth d lifted into its camera, moved by [R | t]
__device__ __forceinline__ void lift_transform(float u, float v, float d, float fx, float fy, float cx, float cy,
                                               const float* R, const float* t, float P[3]) {
  const float X0 = ((u - cx) / fx) * d, X1 = ((v - cy) / fy) * d;
#pragma unroll
  for (int r = 0; r < 3; ++r) P[r] = R[3 * r] * X0 + R[3 * r + 1] * X1 + R[3 * r + 2] * d + t[r];
}

__global__ __launch_bounds__(kReconThreads) void depth_fusion_kernel(
    const float* __restrict__ depth_ref, const float* __restrict__ depth_src, const float* __restrict__ K,
    const float* __restrict__ extr_ref, const float* __restrict__ extr_src, int S, int B, int H, int W,
    float thres_p_dist, float thres_d_diff, int thres_view, unsigned char* __restrict__ count,
    float* __restrict__ fused, int* __restrict__ rec_pixel, unsigned char* __restrict__ rec_consistent) {
  // per view: [R | t] of ref camera -> source camera, then of the way back
  __shared__ float pose[kFusionMaxViews][24];
  const int b = blockIdx.y;
  if ((int)threadIdx.x < S) {
    const float* Er = extr_ref + (size_t)b * 16;
    const float* Es = extr_src + ((size_t)threadIdx.x * B + b) * 16;
    relative_pose(Es, Er, &pose[threadIdx.x][0], &pose[threadIdx.x][9]);
    relative_pose(Er, Es, &pose[threadIdx.x][12], &pose[threadIdx.x][21]);
  }
  __syncthreads();
  const int HW = H * W;
  const int p = blockIdx.x * kReconThreads + threadIdx.x;   // H*W < 2^31 - 256 (checked by the caller)
  if (p >= HW) return;
  const float* Kb = K + (size_t)b * 9;
  const float fx = Kb[0], fy = Kb[4], cx = Kb[2], cy = Kb[5];
  const size_t base = (size_t)b * HW;
  const int yi = p / W, xi = p - yi * W;
  const float x = (float)xi, y = (float)yi;
  const float d = depth_ref[base + p];
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
  float sum = 0.f;
  int n = 0;
  for (int s = 0; s < S; ++s) {
    const float* M = pose[s];
    float P[3];
    lift_transform(x, y, d, fx, fy, cx, cy, M, M + 9, P);
    const float z = fmaxf(P[2], 1e-10f);
    const float u = (fx * P[0] + cx * P[2]) / z, v = (fy * P[1] + cy * P[2]) / z;
    // grid_sample(nearest, align_corners=True, zeros): round half to even; the
    // range test is made in float (|u| may be huge or NaN: then outside)
    const float ur = rintf(u), vr = rintf(v);
    const bool inside = ur >= 0.f && ur <= wm1 && vr >= 0.f && vr <= hm1;
    const size_t view = ((size_t)s * B + b) * HW;
    const float sd = inside ? depth_src[view + (size_t)((int)vr * W + (int)ur)] : 0.f;
    float Q[3];
    lift_transform(u, v, sd, fx, fy, cx, cy, M + 12, M + 21, Q);
    const float d_re = sd > 0.f ? Q[2] : Q[2] * 0.f;
    const float zr = fmaxf(Q[2], 1e-10f);
    const float u_re = (fx * Q[0] + cx * Q[2]) / zr, v_re = (fy * Q[1] + cy * Q[2]) / zr;
    const float du = u_re - x, dv = v_re - y;
    const float dist = sqrtf(du * du + dv * dv);
    const float rel = fabsf(d_re - d) / fmaxf(d, 1e-10f);
    const bool ok = dist < thres_p_dist && rel < thres_d_diff;   // false on NaN
    if (ok) {
      sum += d_re;
      ++n;
    }
    if (rec_pixel) rec_pixel[view + p] = inside ? pack_cell(ur, vr) : kFusionOutside;
    if (rec_consistent) rec_consistent[view + p] = ok ? 1 : 0;
  }
  count[base + p] = (unsigned char)n;
  fused[base + p] = n >= thres_view ? (sum + d) / (float)(n + 1) : 0.f;
}

// ---------------------------------------------------------------- backproject_points
// Valid pixels (depth > 0) of one kPackTile-pixel tile of the flattened
// [B*H*W] map, counted per block.
__global__ __launch_bounds__(kReconThreads) void backproject_count_kernel(const float* __restrict__ depth, int total,
                                                                          int* __restrict__ block_counts) {
  __shared__ int wave_counts[kPackWaves];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  int c = 0;
#pragma unroll
  for (int k = 0; k < kPackRounds; ++k) {
    const long long i = (long long)blockIdx.x * kPackTile + k * kReconThreads + threadIdx.x;
    const bool valid = i < total && depth[i] > 0.f;
    c += __popcll(__ballot(valid));
  }
  if (lane == 0) wave_counts[wid] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kPackWaves; ++w) s += wave_counts[w];
    block_counts[blockIdx.x] = s;
  }
}

// Writes the points.  compact: a point's slot is the number of valid pixels
// before it in frame-major, row-major order -- the counts of the blocks
// before this one, then of the rounds and waves before the thread's, then the
// lanes below it in the wave's ballot: no atomics, the order is the pixel order.
__global__ __launch_bounds__(kReconThreads) void backproject_write_kernel(
    const float* __restrict__ depth, const float* __restrict__ rgb, const float* __restrict__ K,
    const float* __restrict__ cam2world, int HW, int W, int total, int compact,
    const int* __restrict__ block_counts, float* __restrict__ xyz, float* __restrict__ rgb_out, int* __restrict__ n_out) {
  __shared__ int wave_counts[kPackRounds][kPackWaves];
  __shared__ int partial[kPackWaves];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  bool valid[kPackRounds];
  int below[kPackRounds];
  float dv[kPackRounds];
#pragma unroll
  for (int k = 0; k < kPackRounds; ++k) {
    const long long i = (long long)blockIdx.x * kPackTile + k * kReconThreads + threadIdx.x;
    dv[k] = i < total ? depth[i] : 0.f;
    valid[k] = i < total && (compact ? dv[k] > 0.f : true);
    const unsigned long long m = __ballot(valid[k]);
    below[k] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_counts[k][wid] = __popcll(m);
  }
  int before = 0;
  if (compact) {
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += kReconThreads) before += block_counts[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, kWave);
    if (lane == 0) partial[wid] = before;
  }
  __syncthreads();
  int block_base = 0, block_total = 0;
  if (compact) {
    for (int w = 0; w < kPackWaves; ++w) block_base += partial[w];
  } else {
    block_base = (int)blockIdx.x * kPackTile;   // total < 2^31 (checked by the caller)
  }
  for (int k = 0; k < kPackRounds; ++k) {
    for (int w = 0; w < kPackWaves; ++w) block_total += wave_counts[k][w];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_out = block_base + block_total;
  int slot = block_base;
#pragma unroll
  for (int k = 0; k < kPackRounds; ++k) {
    int mine = slot + below[k];
    for (int w = 0; w < kPackWaves; ++w) {
      if (w < wid) mine += wave_counts[k][w];
      slot += wave_counts[k][w];
    }
    if (!valid[k]) continue;
    const int i = (int)blockIdx.x * kPackTile + k * kReconThreads + threadIdx.x;
    const int b = i / HW, p = i - b * HW;
    const int yi = p / W, xi = p - yi * W;
    const float* Kb = K + (size_t)b * 9;
    float R[9], t[3], P[3];
    load_pose(cam2world + (size_t)b * 16, DRO_POSE_MATRIX, R, t);
    lift_transform((float)xi, (float)yi, dv[k], Kb[0], Kb[4], Kb[2], Kb[5], R, t, P);
    float* o = xyz + (size_t)mine * 3;
    o[0] = P[0];
    o[1] = P[1];
    o[2] = P[2];
    const float* c = rgb + (size_t)b * 3 * HW + p;
    float* oc = rgb_out + (size_t)mine * 3;
    oc[0] = c[0];
    oc[1] = c[HW];
    oc[2] = c[2 * (size_t)HW];
  }
}

static bool bad_threshold(float v) { return !(v >= 0.f); }   // negative or NaN

static bool bad_map(int B, int H, int W) {
  return B < 1 || H < 2 || W < 2 || B > 65535 || (long long)H * W >= (1LL << 31) - kReconThreads;
}

}  // namespace dro

using namespace dro;

extern "C" int dro_depth_clean(const float* depth, int B, int H, int W, float grad_max, float depth_max, int crop_h,
                               int crop_w, float* out, void* stream) {
  if (!depth || !out) {
    set_error("depth_clean: NULL pointer");
    return DRO_E_NULL;
  }
  if (bad_map(B, H, W) || crop_h < 0 || crop_w < 0) {
    set_error("depth_clean: sizes out of range (B 1..65535, H, W >= 2, H*W < 2^31, crop >= 0)");
    return DRO_E_SHAPE;
  }
  if (bad_threshold(grad_max) || bad_threshold(depth_max)) {
    set_error("depth_clean: threshold negative or NaN (grad_max, depth_max)");
    return DRO_E_MODE;
  }
  hipLaunchKernelGGL(depth_clean_kernel, dim3((H * W + kReconThreads - 1) / kReconThreads, B), dim3(kReconThreads),
                     0, (hipStream_t)stream, depth, H, W, grad_max, depth_max, crop_h, crop_w, out);
  return launch_status("depth_clean_kernel launch failed");
}

extern "C" int dro_depth_fusion(const float* depth_ref, const float* depth_src, const float* K,
                                const float* extr_ref, const float* extr_src, int S, int B, int H, int W,
                                float thres_p_dist, float thres_d_diff, int thres_view, unsigned char* count,
                                float* fused, int* rec_pixel, unsigned char* rec_consistent, void* stream) {
  if (!depth_ref || !depth_src || !K || !extr_ref || !extr_src || !count || !fused) {
    set_error("depth_fusion: NULL pointer");
    return DRO_E_NULL;
  }
  if (bad_map(B, H, W) || S < 1 || S > kFusionMaxViews) {
    set_error("depth_fusion: sizes out of range (S 1..8, B 1..65535, H, W >= 2, H*W < 2^31)");
    return DRO_E_SHAPE;
  }
  if (bad_threshold(thres_p_dist) || bad_threshold(thres_d_diff) || thres_view < 0) {
    set_error("depth_fusion: threshold negative or NaN (thres_p_dist, thres_d_diff, thres_view)");
    return DRO_E_MODE;
  }
  hipLaunchKernelGGL(depth_fusion_kernel, dim3((H * W + kReconThreads - 1) / kReconThreads, B), dim3(kReconThreads),
                     0, (hipStream_t)stream, depth_ref, depth_src, K, extr_ref, extr_src, S, B, H, W, thres_p_dist,
                     thres_d_diff, thres_view, count, fused, rec_pixel, rec_consistent);
  return launch_status("depth_fusion_kernel launch failed");
}

static bool bad_cloud(int B, int H, int W) {
  return B < 1 || H < 2 || W < 2 || (long long)B * H * W >= (1LL << 31) - kPackTile;
}

extern "C" size_t dro_backproject_points_workspace_bytes(int B, int H, int W) {
  if (bad_cloud(B, H, W)) return 0;
  const long long total = (long long)B * H * W;
  return (size_t)((total + kPackTile - 1) / kPackTile) * sizeof(int);
}

extern "C" int dro_backproject_points(const float* depth, const float* rgb, const float* K, const float* cam2world,
                                      int B, int H, int W, int keep_invalid, float* xyz, float* rgb_out, int* n,
                                      void* workspace, void* stream) {
  if (!depth || !rgb || !K || !cam2world || !xyz || !rgb_out || !n || (!keep_invalid && !workspace)) {
    set_error("backproject_points: NULL pointer");
    return DRO_E_NULL;
  }
  if (bad_cloud(B, H, W)) {
    set_error("backproject_points: sizes out of range (B >= 1, H, W >= 2, B*H*W < 2^31)");
    return DRO_E_SHAPE;
  }
  const int total = B * H * W;
  const int nblk = (total + kPackTile - 1) / kPackTile;
  int* counts = (int*)workspace;
  if (!keep_invalid) {
    hipLaunchKernelGGL(backproject_count_kernel, dim3(nblk), dim3(kReconThreads), 0, (hipStream_t)stream, depth,
                       total, counts);
    const int st = launch_status("backproject_count_kernel launch failed");
    if (st) return st;
  }
  hipLaunchKernelGGL(backproject_write_kernel, dim3(nblk), dim3(kReconThreads), 0, (hipStream_t)stream, depth, rgb,
                     K, cam2world, H * W, W, total, keep_invalid ? 0 : 1, counts, xyz, rgb_out, n);
  return launch_status("backproject_write_kernel launch failed");
}
