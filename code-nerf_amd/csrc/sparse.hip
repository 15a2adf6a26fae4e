// Occupancy-grid rendering: build the grid, mark / gather the samples that fall
// in occupied cells, scatter the compact MLP outputs back to the dense arrays.
// No reference counterpart (the reference evaluates the MLP at every sample);
// DESIGN.md 8.4 has the definition.
//
// The grid is G^3 cells over the box [lo, lo + G / inv_cell)^3, one bit per
// cell: cell c = (ix G + iy) G + iz is bit c & 31 of word c >> 5.  A sample s
// of ray r is KEPT when its point, formed with the chain prologue's separately
// rounded operations,
//   x_a = o_a + d_a z,   t_a = (x_a - lo_a) inv_cell,   0 <= t_a < G  (NaN: no)
// falls in a set cell i_a = floor(t_a), or when it is the ray's last sample and
// keep_last is set.  keep[r][8]: bit s & 31 of word s >> 5 (N <= 256).
//
// One wave per ray, 4 rays per block, as the compositing kernels: a sample's
// rank among the kept samples of its ray is a popcount of the ballot below it.
// No atomics; every output is written by exactly one lane.
#include "cn_common.h"

namespace cn {

constexpr int kKeepWords = 8;          // keep words per ray: 256 samples

// One thread per output word: the 32 cells (ix, iy, iz0 .. iz0 + 31).  col bit j
// says whether any cell (x', y', iz0 - dilate + j) with |x' - ix|, |y' - iy| <=
// dilate is occupied (sigma >= tau, NaN occupied; outside the box: not); the
// cell's bit is the OR of the 2 dilate + 1 column bits around it.
__global__ __launch_bounds__(256) void occupancy_build_kernel(const float* __restrict__ sigma, int G, float tau,
                                                              int dilate, uint32_t* __restrict__ bits) {
  const int wpr = G >> 5;                                   // words per z row
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= G * G * wpr) return;
  const int iz0 = (w % wpr) << 5;
  const int iy = (w / wpr) % G;
  const int ix = w / (wpr * G);
  const int x0 = max(ix - dilate, 0), x1 = min(ix + dilate, G - 1);
  const int y0 = max(iy - dilate, 0), y1 = min(iy + dilate, G - 1);
  const int nz = 32 + 2 * dilate;                           // <= 40 column bits
  uint64_t col = 0;
  for (int x = x0; x <= x1; ++x)
    for (int y = y0; y <= y1; ++y) {
      const float* row = sigma + ((size_t)x * G + y) * G;
      for (int j = 0; j < nz; ++j) {
        const int z = iz0 - dilate + j;
        if (z >= 0 && z < G && !(row[z] < tau)) col |= 1ull << j;
      }
    }
  uint64_t out = 0;
  for (int k = 0; k <= 2 * dilate; ++k) out |= col >> k;
  bits[w] = (uint32_t)out;
}

struct SparseGrid {
  const uint32_t* bits;
  int G;
  float lo[3], inv_cell;
};

CN_DEV bool cell_set(const SparseGrid& g, const float o[3], const float d[3], float z) {
  int i[3];
  const float Gf = (float)g.G;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float x = fadd_rn(o[a], fmul_rn(d[a], z));
    const float t = fmul_rn(fadd_rn(x, -g.lo[a]), g.inv_cell);
    if (!(t >= 0.f && t < Gf)) return false;
    i[a] = (int)t;                                          // floor: t >= 0
  }
  const uint32_t c = ((uint32_t)i[0] * g.G + i[1]) * g.G + i[2];
  return (g.bits[c >> 5] >> (c & 31)) & 1u;
}

__global__ __launch_bounds__(256) void sparse_mark_kernel(const float* __restrict__ ro, const float* __restrict__ rd,
                                                          const float* __restrict__ z, int z_stride, int R, int N,
                                                          SparseGrid g, int keep_last, uint32_t* __restrict__ keep,
                                                          int* __restrict__ count) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int lane = threadIdx.x & 63;
  const float o[3] = {ro[3 * r], ro[3 * r + 1], ro[3 * r + 2]};
  const float d[3] = {rd[3 * r], rd[3 * r + 1], rd[3 * r + 2]};
  const float* zr = z + (size_t)r * z_stride;
  uint32_t mine = 0;        // lane l < 8 ends up holding keep word l
  int total = 0;
#pragma unroll
  for (int i = 0; i < kKeepWords / 2; ++i) {
    const int s = i * 64 + lane;
    bool k = false;
    if (s < N) k = (keep_last && s == N - 1) || cell_set(g, o, d, zr[s]);
    const uint64_t m = __ballot(k);
    total += __popcll(m);
    if (lane == 2 * i) mine = (uint32_t)m;
    if (lane == 2 * i + 1) mine = (uint32_t)(m >> 32);
  }
  if (lane < kKeepWords) keep[(size_t)r * kKeepWords + lane] = mine;
  if (lane == 0) count[r] = total;
}

// this lane's sample s = i * 64 + lane: kept?  *rank = kept samples of the ray
// before it.  kw: the ray's keep words, `before` the kept samples of the earlier
// 64-sample groups (updated).
CN_DEV bool kept_rank(const uint32_t* kw, int i, int lane, int* before, int* rank) {
  const uint64_t m = (uint64_t)kw[2 * i] | ((uint64_t)kw[2 * i + 1] << 32);
  *rank = *before + __popcll(m & ((1ull << lane) - 1ull));
  *before += __popcll(m);
  return (m >> lane) & 1ull;
}

__global__ __launch_bounds__(256) void sparse_gather_kernel(const float* __restrict__ ro, const float* __restrict__ rd,
                                                            const float* __restrict__ z, int z_stride, int R, int N,
                                                            const uint32_t* __restrict__ keep,
                                                            const int* __restrict__ offset, float* __restrict__ xyz,
                                                            float* __restrict__ vdir) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int lane = threadIdx.x & 63;
  const uint32_t* kw = keep + (size_t)r * kKeepWords;
  const float* zr = z + (size_t)r * z_stride;
  const int off = offset[r];
  int before = 0;
#pragma unroll
  for (int i = 0; i < kKeepWords / 2; ++i) {
    const int s = i * 64 + lane;
    int rank;
    const bool k = kept_rank(kw, i, lane, &before, &rank);
    if (s < N && k) {
      const size_t m = (size_t)off + rank;
      const float zz = zr[s];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float d = rd[3 * r + a];
        xyz[3 * m + a] = fadd_rn(ro[3 * r + a], fmul_rn(d, zz));
        vdir[3 * m + a] = d;
      }
    }
  }
}

__global__ __launch_bounds__(256) void sparse_scatter_kernel(const uint32_t* __restrict__ keep,
                                                             const int* __restrict__ offset, int R, int N,
                                                             const float* __restrict__ sigma_k,
                                                             const float* __restrict__ rgb_k,
                                                             float* __restrict__ sigma, float* __restrict__ rgb) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int lane = threadIdx.x & 63;
  const uint32_t* kw = keep + (size_t)r * kKeepWords;
  const int off = offset[r];
  int before = 0;
#pragma unroll
  for (int i = 0; i < kKeepWords / 2; ++i) {
    const int s = i * 64 + lane;
    int rank;
    const bool k = kept_rank(kw, i, lane, &before, &rank);
    if (s >= N) continue;
    const size_t n = (size_t)r * N + s;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (k) {
      const size_t m = (size_t)off + rank;
      v[0] = sigma_k[m];
      v[1] = rgb_k[3 * m];
      v[2] = rgb_k[3 * m + 1];
      v[3] = rgb_k[3 * m + 2];
    }
    sigma[n] = v[0];
    rgb[3 * n] = v[1];
    rgb[3 * n + 1] = v[2];
    rgb[3 * n + 2] = v[3];
  }
}

}  // namespace cn
