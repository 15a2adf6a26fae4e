// Evaluation metrics of the test-time loop on the device: the PSNR argument
// (mean of the chunk MSEs, reference src/optimizer.py:117-125) and SSIM as
// codenerf_amd.metrics.ssim_legacy defines it (skimage's
// structural_similarity(multichannel=True) as src/optimizer.py:156 calls it).
//
// SSIM: per channel a 7x7 uniform window, sample covariance (49/48),
// C1 = (0.01 * 2)^2, C2 = (0.03 * 2)^2, the mean of S over the image cropped by
// 3 on every side, then the mean over the 3 channels.  After that crop every
// window lies inside the image, so the border mode of the uniform filter
// (scipy's 'reflect') never enters the result and the kernel has NO border
// handling: it sums the (H - 6) x (W - 6) valid windows only.  Window sums, S
// and every reduction are float64 (an fp32 restatement was off by 2e-8 on a
// white-background image).
//
// metrics_partial_kernel, grid (tiles + segments, V):
//   blocks [0, tiles): one 32 x 8 tile of windows.  The tile's pixels and
//     their 6-pixel halo (38 x 14, both images, channels interleaved as in
//     memory) are staged in LDS; one thread per window (lane = column, so the
//     32 lanes of a bank group read dwords 3 apart: conflict-free); the
//     block's sum of S over windows and channels goes to the workspace.
//   blocks [tiles, tiles + segments): one segment of <= 1024 rays of one
//     chunk: sum of (img - gt)^2, converted to float64 before the subtraction.
// metrics_final_kernel, grid (V): thread c sums the segments of chunk c in
//   order and divides by 3 n_c (the chunk mean, written to d_chunk_mse); the
//   chunk means and the tile sums are then summed over the block.
// Every block sum is a fixed xor butterfly per wave and a fixed order over the
// waves: no atomics, deterministic, and a view's numbers depend on its own
// blocks only (not on V or on the views beside it).
#include "cn_ray.h"

namespace cn {

constexpr int kMetTileW = 32, kMetTileH = 8;          // windows per block
constexpr int kMetWin = 7, kMetHalo = kMetWin - 1;
constexpr int kMetInW = kMetTileW + kMetHalo, kMetInH = kMetTileH + kMetHalo;
constexpr int kMetRowF = kMetInW * 3;                 // floats per staged row
constexpr int kMetBlock = kMetTileW * kMetTileH;      // 256
constexpr int kMetSeg = 1024;                         // rays per MSE segment

// Host and device agree on the launch geometry through this one struct.
struct MetricsGeom {
  int H, W, chunk;        // chunk clamped to H * W (one chunk either way)
  int tiles_x, tiles;     // SSIM tiles per view
  int nchunk, spc;        // chunks per view, segments per chunk
  __host__ __device__ int parts() const { return tiles + nchunk * spc; }
};

inline MetricsGeom metrics_geom(int H, int W, int chunk) {
  MetricsGeom g;
  const int HW = H * W;
  g.H = H, g.W = W;
  g.chunk = chunk < HW ? chunk : HW;
  g.tiles_x = (W - kMetHalo + kMetTileW - 1) / kMetTileW;
  g.tiles = g.tiles_x * ((H - kMetHalo + kMetTileH - 1) / kMetTileH);
  g.nchunk = (HW + g.chunk - 1) / g.chunk;
  g.spc = (g.chunk + kMetSeg - 1) / kMetSeg;
  return g;
}

// Sum over the 256 threads of a block, the same value in every thread of wave
// 0 .. 3 after the call; `red` is 4 doubles of LDS.
CN_DEV double metrics_block_sum(double s, double* red) {
  s = wave_sum(s);
  __syncthreads();                       // red may still be read from an earlier sum
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double tot = 0.0;
#pragma unroll
  for (int k = 0; k < kMetBlock / 64; ++k) tot += red[k];
  return tot;
}

__global__ __launch_bounds__(kMetBlock) void metrics_partial_kernel(const float* __restrict__ img,
                                                                    const float* __restrict__ gt, MetricsGeom g,
                                                                    double* __restrict__ ws) {
  __shared__ float tile[2][kMetInH * kMetRowF];
  __shared__ double red[kMetBlock / 64];
  const int v = blockIdx.y, b = blockIdx.x;
  const size_t view = (size_t)v * g.H * g.W * 3;      // 64-bit: V * H * W * 3 may pass 2^31
  const float* a = img + view;
  const float* r = gt + view;
  double* out = ws + (size_t)v * g.parts() + b;
  double s = 0.0;
  if (b < g.tiles) {
    const int ty0 = (b / g.tiles_x) * kMetTileH, tx0 = (b % g.tiles_x) * kMetTileW;
    // rows of the staged tile are contiguous in memory: [col][3]
    const int row_f = min(kMetInW, g.W - tx0) * 3;    // floats of a row inside the image
    for (int e = threadIdx.x; e < kMetInH * kMetRowF; e += kMetBlock) {
      const int row = e / kMetRowF, k = e - row * kMetRowF;
      float x = 0.f, y = 0.f;
      if (ty0 + row < g.H && k < row_f) {
        const int at = ((ty0 + row) * g.W + tx0) * 3 + k;   // < 3 H W <= 3 * 2^28
        x = a[at], y = r[at];
      }
      tile[0][e] = x, tile[1][e] = y;
    }
    __syncthreads();
    const int lx = threadIdx.x % kMetTileW, ly = threadIdx.x / kMetTileW;
    if (tx0 + lx < g.W - kMetHalo && ty0 + ly < g.H - kMetHalo) {
      double sx[3] = {}, sy[3] = {}, sxx[3] = {}, syy[3] = {}, sxy[3] = {};
      for (int dy = 0; dy < kMetWin; ++dy) {
        const int base = (ly + dy) * kMetRowF + lx * 3;
#pragma unroll
        for (int dx = 0; dx < kMetWin; ++dx) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double x = (double)tile[0][base + dx * 3 + c], y = (double)tile[1][base + dx * 3 + c];
            sx[c] += x, sy[c] += y;
            sxx[c] += x * x, syy[c] += y * y, sxy[c] += x * y;
          }
        }
      }
      constexpr double n = kMetWin * kMetWin, cov = n / (n - 1.0);
      constexpr double C1 = (0.01 * 2.0) * (0.01 * 2.0), C2 = (0.03 * 2.0) * (0.03 * 2.0);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double ux = sx[c] / n, uy = sy[c] / n;
        const double vx = cov * (sxx[c] / n - ux * ux), vy = cov * (syy[c] / n - uy * uy);
        const double vxy = cov * (sxy[c] / n - ux * uy);
        s += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
      }
    }
  } else {
    const int q = b - g.tiles, c = q / g.spc, seg = q - c * g.spc;
    const int HW = g.H * g.W;
    const int r0 = c * g.chunk + seg * kMetSeg;                       // first ray of the segment
    const int r1 = min(min(r0 + kMetSeg, (c + 1) * g.chunk), HW);     // a ragged last chunk: maybe none
    for (int e = r0 * 3 + threadIdx.x; e < r1 * 3; e += kMetBlock) {
      const double d = (double)a[e] - (double)r[e];
      s += d * d;
    }
  }
  const double tot = metrics_block_sum(s, red);
  if (threadIdx.x == 0) *out = tot;
}

__global__ __launch_bounds__(kMetBlock) void metrics_final_kernel(const double* __restrict__ ws, MetricsGeom g,
                                                                  double* __restrict__ out,
                                                                  double* __restrict__ chunk_mse) {
  __shared__ double red[kMetBlock / 64];
  const int v = blockIdx.x;
  const double* part = ws + (size_t)v * g.parts();
  const int HW = g.H * g.W;
  double means = 0.0;
  for (int c = threadIdx.x; c < g.nchunk; c += kMetBlock) {
    double s = 0.0;
    for (int k = 0; k < g.spc; ++k) s += part[g.tiles + (size_t)c * g.spc + k];
    const int n = min(g.chunk, HW - c * g.chunk);
    const double m = s / (3.0 * (double)n);
    if (chunk_mse) chunk_mse[(size_t)v * g.nchunk + c] = m;
    means += m;
  }
  const double mse = metrics_block_sum(means, red) / (double)g.nchunk;
  double ss = 0.0;
  for (int t = threadIdx.x; t < g.tiles; t += kMetBlock) ss += part[t];
  const double ssim = metrics_block_sum(ss, red) / (3.0 * (double)(g.H - kMetHalo) * (double)(g.W - kMetHalo));
  if (threadIdx.x == 0) {
    out[2 * (size_t)v] = mse;
    out[2 * (size_t)v + 1] = ssim;
  }
}

}  // namespace cn
