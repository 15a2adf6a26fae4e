// Several objects in one picture (no reference counterpart).
//
// A scene is K <= 8 objects, each with its own codes, occupancy grid and a
// similarity transform object -> world (rotation R, translation t, scale s).
// Three kernels, the rest of the schedule being the existing entries:
//   scene_rays_kernel       the world rays in every object's frame,
//   scene_combine_kernel    the K density / colour planes as one,
//   scene_composite_kernel  composite_fwd_kernel / composite_fine_fwd_kernel on
//                           the combined planes, plus the ray's weights split
//                           back onto the objects and the instance label.
// Every float32 operation below is rounded separately (fmul_rn / fadd_rn, no
// contraction; `/` is the correctly rounded division) in the order written, so
// that tests/scene_util.py restates them bit for bit.  No atomics; every output
// element is written by exactly one lane.
#include "cn_ray.h"

namespace cn {

constexpr int kMaxObjects = 8;

// by-value kernel arguments: the host arrays are read at the call
struct SceneXf {
  float R[9];                           // object -> world rotation, row-major
  float t[3];
  float inv_s;
};
struct SceneXfs {
  SceneXf x[kMaxObjects];
};
struct SceneInvS {
  float v[kMaxObjects];
};

// o_k = R^T (o - t) / s, d_k = R^T d (not re-normalised).  blockIdx.y is the
// object, so its transform is read through scalar loads.
__global__ __launch_bounds__(256) void scene_rays_kernel(const float* __restrict__ ro, const float* __restrict__ rd,
                                                         int R, SceneXfs xf, float* __restrict__ out_o,
                                                         float* __restrict__ out_d) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const SceneXf& x = xf.x[blockIdx.y];
  const size_t dst = ((size_t)blockIdx.y * R + r) * 3;
  float q[3], d[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    q[b] = fadd_rn(ro[3 * (size_t)r + b], -x.t[b]);
    d[b] = rd[3 * (size_t)r + b];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float qo = fadd_rn(fadd_rn(fmul_rn(x.R[a], q[0]), fmul_rn(x.R[3 + a], q[1])), fmul_rn(x.R[6 + a], q[2]));
    out_o[dst + a] = fmul_rn(qo, x.inv_s);
    out_d[dst + a] = fadd_rn(fadd_rn(fmul_rn(x.R[a], d[0]), fmul_rn(x.R[3 + a], d[1])), fmul_rn(x.R[6 + a], d[2]));
  }
}

// The share of object k in a sample of combined density sigma: a / sigma with
// a = sigma_k / s_k, 0 unless sigma > 0 (a NaN sum included).
CN_DEV float scene_share(float sigma_k, float inv_s, float sigma) {
  return sigma > 0.f ? fmul_rn(sigma_k, inv_s) / sigma : 0.f;
}

// sigma = sum_k a_k, rgb = sum_k (a_k / sigma) rgb_k, both left to right.
__global__ __launch_bounds__(256) void scene_combine_kernel(const float* __restrict__ sig_k,
                                                            const float* __restrict__ rgb_k, SceneInvS inv_s, int K,
                                                            int M, float* __restrict__ sig, float* __restrict__ rgb) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float s[kMaxObjects];
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxObjects; ++k) {
    if (k < K) {
      s[k] = sig_k[(size_t)k * M + m];
      const float a = fmul_rn(s[k], inv_s.v[k]);
      sum = k == 0 ? a : fadd_rn(sum, a);
    }
  }
  float c[3] = {0.f, 0.f, 0.f};
  if (sum > 0.f) {
#pragma unroll
    for (int k = 0; k < kMaxObjects; ++k) {
      if (k < K) {
        const float f = scene_share(s[k], inv_s.v[k], sum);
        const float* p = rgb_k + ((size_t)k * M + m) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float v = fmul_rn(f, p[i]);
          c[i] = k == 0 ? v : fadd_rn(c[i], v);
        }
      }
    }
  }
  sig[m] = sum;
  rgb[3 * (size_t)m + 0] = c[0];
  rgb[3 * (size_t)m + 1] = c[1];
  rgb[3 * (size_t)m + 2] = c[2];
}

struct SceneCompositeArgs {
  MergePlanes p;                        // the combined planes; sig_f, rgb_f, zf NULL when Nf == 0
  const float *obj_c, *obj_f;           // [K][R*Nc], [K][R*Nf]; read only with labels
  SceneInvS inv_s;
  int K, R, white_bg;
  float acc_min;
  float *out_rgb, *out_depth, *out_acc; // required
  float* obj_acc;                       // [R][K] or NULL
  int* instance;                        // [R] or NULL, together with obj_acc
};

// One wave per ray, 4 rays per block, as composite_aov_kernel: merge_ray with
// the source of every merged slot kept, ray_forward / ray_reduce, then per
// object sum_i w_i f_k,i.
template <bool kMerge>
__global__ __launch_bounds__(256) void scene_composite_kernel(SceneCompositeArgs a) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wv;
  if (r >= a.R) return;                     // wave-uniform; only wave-level sync below
  const int Nc = a.p.Nc, Nf = a.p.Nf;
  const bool labels = a.obj_acc != nullptr;
  RayState st;
  int src[kMaxPer];                         // coarse i: i, fine j: Nc + j, nothing: -1
  if constexpr (kMerge) {
    // 4 waves x 256 slots x 7 words = 28 KiB
    __shared__ float m_sig[4][kMaxRaySamples], m_z[4][kMaxRaySamples], m_rgb[4][kMaxRaySamples * 3];
    __shared__ float z_stage[4][kMaxRaySamples];
    __shared__ int m_src[4][kMaxRaySamples];
    // the source indexes obj_c / obj_f below
    merge_ray<true>(a.p, r, MergeRows{m_sig[wv], m_z[wv], m_rgb[wv], m_src[wv]}, z_stage[wv]);
    ray_forward(st, m_sig[wv], m_rgb[wv], m_z[wv], Nc + Nf);
#pragma unroll
    for (int k = 0; k < kMaxPer; ++k) src[k] = k < st.cnt ? m_src[wv][st.n0 + k] : -1;
  } else {
    ray_forward(st, a.p.sig_c + (size_t)r * Nc, a.p.rgb_c + (size_t)r * Nc * 3, a.p.zc + (size_t)r * a.p.zc_stride, Nc);
#pragma unroll
    for (int k = 0; k < kMaxPer; ++k) src[k] = k < st.cnt ? st.n0 + k : -1;
  }
  float o[5];
  ray_reduce(st, o);
  store_ray(o, r, a.white_bg, a.out_rgb, a.out_depth, a.out_acc);
  if (!labels) return;
  const size_t Mc = (size_t)a.R * Nc, Mf = (size_t)a.R * Nf;
  int best = 0;
  float best_acc = 0.f;
#pragma unroll
  for (int ko = 0; ko < kMaxObjects; ++ko) {
    if (ko < a.K) {
      const float inv_s = a.inv_s.v[ko];
      double part = 0.0;
#pragma unroll
      for (int k = 0; k < kMaxPer; ++k) {
        const int s = src[k];
        if (s >= 0) {
          const float sk = s < Nc ? a.obj_c[ko * Mc + (size_t)r * Nc + s] : a.obj_f[ko * Mf + (size_t)r * Nf + (s - Nc)];
          part += (double)fmul_rn(st.w[k], scene_share(sk, inv_s, st.sig[k]));
        }
      }
      const float oa = (float)wave_sum(part);
      if (lane == 0) a.obj_acc[(size_t)r * a.K + ko] = oa;
      if (ko == 0 || oa > best_acc) {       // strictly greater: a tie stays with the lower index
        best = ko;
        best_acc = oa;
      }
    }
  }
  if (lane == 0) a.instance[r] = o[4] >= a.acc_min ? best : -1;
}

}  // namespace cn
