// Geometry buffers of a composited ray (no reference counterpart; DESIGN.md
// 8.6): next to the rgb, expected depth and opacity that ray_reduce gives, the
// median depth and the weighted normal.
//
// Over a ray's samples k = 0 .. N-1 (the merged coarse + fine samples with
// Nf > 0, by the rule of merge_ray) with the weights w_k that
// ray_forward leaves in RayState:
//   depth_med = z_m for the first m with C_m >= 0.5, C_k = sum_{j <= k} (double)
//               w_j in sample order; z_{N-1} when no such m exists;
//   normal    = sum_k w_k u_k (not normalised: its length is at most the
//               opacity), u_k = -g_k / |g_k| in fp32 with g_k = d sigma / d xyz
//               of the sample, (0, 0, 0) unless |g_k| > 0 (mesh.unit_normals);
//               products rounded to fp32, summed in float64 in a fixed order
//               and rounded once, as ray_reduce does.
// One wave per ray, 4 rays per block, as the compositing kernels of render.hip,
// with the same ray_forward / ray_reduce (cn_ray.h): rgb, depth and opacity are
// cn_composite_fwd's / cn_composite_fine_fwd's bit for bit.  No atomics; every
// output element is written by exactly one lane.
#include "cn_ray.h"

namespace cn {

struct AovArgs {
  MergePlanes p;                        // sig_f, rgb_f, zf NULL when Nf == 0
  const float* grad_c;                  // [R*Nc][3] or NULL
  const float* grad_f;                  // [R*Nf][3] or NULL
  int R, white_bg;
  float *out_rgb, *out_depth;           // required
  float *out_acc, *out_med;             // [R], each may be NULL
  float* out_normal;                    // [R][3] or NULL (then no gradient is read)
};

// u = -g / |g|; (0, 0, 0) unless |g| > 0 (a zero or NaN gradient).  |g| as
// torch forms it elementwise: ((x x + y y) + z z) separately rounded, sqrt.
CN_DEV void unit_normal(const float* g, float u[3]) {
  const float x = g[0], y = g[1], z = g[2];
  const float n = sqrtf(fadd_rn(fadd_rn(fmul_rn(x, x), fmul_rn(y, y)), fmul_rn(z, z)));
  const bool ok = n > 0.f;
  u[0] = ok ? -x / n : 0.f;
  u[1] = ok ? -y / n : 0.f;
  u[2] = ok ? -z / n : 0.f;
}

template <bool kMerge>
__global__ __launch_bounds__(256) void composite_aov_kernel(AovArgs a) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wv;
  if (r >= a.R) return;                     // wave-uniform; only wave-level sync below
  const int Nc = a.p.Nc, N = Nc + a.p.Nf;
  const bool nrm = a.out_normal != nullptr;
  RayState st;
  float u[kMaxPer][3];
  if constexpr (kMerge) {
    // 4 waves x 256 slots x 9 floats = 36 KiB
    __shared__ float m_sig[4][kMaxRaySamples], m_z[4][kMaxRaySamples], m_rgb[4][kMaxRaySamples * 3];
    __shared__ float m_u[4][kMaxRaySamples * 3], z_stage[4][kMaxRaySamples];
    // no source table: the normals travel with their merged slot
    merge_ray<false>(a.p, r, MergeRows{m_sig[wv], m_z[wv], m_rgb[wv], nullptr}, z_stage[wv],
                     [&](int p, bool fine, size_t g) {
                       if (nrm) unit_normal((fine ? a.grad_f : a.grad_c) + 3 * g, &m_u[wv][3 * p]);
                     });
    ray_forward(st, m_sig[wv], m_rgb[wv], m_z[wv], N);
    if (nrm) {
#pragma unroll
      for (int k = 0; k < kMaxPer; ++k)
        if (k < st.cnt)
          for (int c = 0; c < 3; ++c) u[k][c] = m_u[wv][3 * (st.n0 + k) + c];
    }
  } else {
    ray_forward(st, a.p.sig_c + (size_t)r * Nc, a.p.rgb_c + (size_t)r * Nc * 3, a.p.zc + (size_t)r * a.p.zc_stride, Nc);
    if (nrm) {
#pragma unroll
      for (int k = 0; k < kMaxPer; ++k)
        if (k < st.cnt) unit_normal(a.grad_c + ((size_t)r * Nc + st.n0 + k) * 3, u[k]);
    }
  }
  float o[5];
  ray_reduce(st, o);
  store_ray(o, r, a.white_bg, a.out_rgb, a.out_depth, a.out_acc);
  if (a.out_med) {
    // C_k: the lanes own consecutive runs of samples, so the lane order is the
    // sample order -- prefix over the lanes, then along the lane's own run
    double part = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxPer; ++k)
      if (k < st.cnt) part += (double)st.w[k];
    double run = wave_inclusive_sum(part) - part;
    int m = N;                              // this lane's first sample with C >= 0.5
#pragma unroll
    for (int k = 0; k < kMaxPer; ++k) {
      if (k < st.cnt) {
        run += (double)st.w[k];
        if (m == N && run >= 0.5) m = st.n0 + k;
      }
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) m = min(m, __shfl_xor(m, k));
    if (m == N) m = N - 1;                  // never reached (NaN weights included)
#pragma unroll
    for (int k = 0; k < kMaxPer; ++k)
      if (k < st.cnt && st.n0 + k == m) a.out_med[r] = st.z[k];
  }
  if (nrm) {
    double acc[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < kMaxPer; ++k) {
      if (k < st.cnt) {
        acc[0] += (double)fmul_rn(st.w[k], u[k][0]);
        acc[1] += (double)fmul_rn(st.w[k], u[k][1]);
        acc[2] += (double)fmul_rn(st.w[k], u[k][2]);
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double v = wave_sum(acc[i]);
      if (lane == 0) a.out_normal[3 * r + i] = (float)v;
    }
  }
}

}  // namespace cn
