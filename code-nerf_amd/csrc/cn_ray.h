// Ray-level device code shared by the compositing kernels (render.hip,
// aov.hip, scene.hip) and the wave primitives that metrics.hip and
// inputgrad.hip use as well.
//
// One wave per ray: lane l owns a contiguous run of samples, the exclusive
// transmittance product and the reverse cumulative sum are wave scans.  Both
// accumulate in float64, as torch's CPU cumprod/cumsum do (acc_type<float> is
// double on the CPU), so the rounded float results match the reference.
#pragma once
#include "cn_common.h"

namespace cn {

// ---------------------------------------------------------------- wave primitives
CN_DEV double shfl_xor_d(double v, int k) {
  return __hiloint2double(__shfl_xor(__double2hiint(v), k), __shfl_xor(__double2loint(v), k));
}
CN_DEV double shfl_up_d(double v, int k) {
  const int lo = __shfl_up(__double2loint(v), k);
  const int hi = __shfl_up(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}
CN_DEV double shfl_down_d(double v, int k) {
  const int lo = __shfl_down(__double2loint(v), k);
  const int hi = __shfl_down(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}
// sum over the wave by a fixed xor butterfly: the same value in every lane
CN_DEV double wave_sum(double v) {
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) v += shfl_xor_d(v, k);
  return v;
}
// inclusive prefix sum over lanes
CN_DEV double wave_inclusive_sum(double v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const double o = shfl_up_d(v, k);
    if (lane >= k) v += o;
  }
  return v;
}
// exclusive product over lanes (lane 0 gets 1)
CN_DEV double wave_exclusive_prod(double v) {
  const int lane = threadIdx.x & 63;
  double incl = v;
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const double o = shfl_up_d(incl, k);
    if (lane >= k) incl *= o;
  }
  double ex = shfl_up_d(incl, 1);
  return lane == 0 ? 1.0 : ex;
}
// exclusive suffix sum over lanes (lane 63 gets 0)
CN_DEV double wave_exclusive_suffix_sum(double v) {
  const int lane = threadIdx.x & 63;
  double incl = v;
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const double o = shfl_down_d(incl, k);
    if (lane + k < 64) incl += o;
  }
  double ex = shfl_down_d(incl, 1);
  return lane == 63 ? 0.0 : ex;
}
// LDS written by some lanes of a wave becomes visible to its other lanes: the
// only synchronisation of the one-wave-per-ray kernels (no block barrier, so
// a wave may leave early)
CN_DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------- one ray
constexpr int kMaxPer = 4;   // samples per lane: N <= 256
constexpr int kMaxRaySamples = 64 * kMaxPer;

struct RayState {
  int n0, cnt;                // this lane's sample range
  float sig[kMaxPer], z[kMaxPer], delta[kMaxPer], e[kMaxPer], alpha[kMaxPer], trans[kMaxPer];
  float T[kMaxPer], w[kMaxPer], c[kMaxPer][3];
};

// Forward of one ray (src/utils.py:35-43), lane-local part + scan.
CN_DEV void ray_forward(RayState& st, const float* sig, const float* rgb, const float* z, int N) {
  const int lane = threadIdx.x & 63;
  const int per = (N + 63) / 64;
  st.n0 = lane * per;
  st.cnt = max(0, min(per, N - st.n0));
  double prod = 1.0;
#pragma unroll
  for (int k = 0; k < kMaxPer; ++k) {
    if (k < st.cnt) {
      const int s = st.n0 + k;
      st.sig[k] = sig[s];
      st.z[k] = z[s];
      st.delta[k] = s + 1 < N ? fadd_rn(z[s + 1], -z[s]) : 1e10f;
      st.e[k] = expf(-fmul_rn(st.sig[k], st.delta[k]));
      st.alpha[k] = 1.f - st.e[k];
      st.trans[k] = fadd_rn(1.f - st.alpha[k], 1e-10f);
      if (rgb) {
        st.c[k][0] = rgb[3 * s + 0];
        st.c[k][1] = rgb[3 * s + 1];
        st.c[k][2] = rgb[3 * s + 2];
      }
      prod *= (double)st.trans[k];
    }
  }
  double run = wave_exclusive_prod(prod);
#pragma unroll
  for (int k = 0; k < kMaxPer; ++k) {
    if (k < st.cnt) {
      st.T[k] = (float)run;
      run *= (double)st.trans[k];
      st.w[k] = fmul_rn(st.alpha[k], st.T[k]);
    }
  }
}

// rgb (3), depth, weight sum of a ray (sums in float64, rounded once)
CN_DEV void ray_reduce(const RayState& st, float out[5]) {
  double acc[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < kMaxPer; ++k) {
    if (k < st.cnt) {
      acc[0] += (double)fmul_rn(st.w[k], st.c[k][0]);
      acc[1] += (double)fmul_rn(st.w[k], st.c[k][1]);
      acc[2] += (double)fmul_rn(st.w[k], st.c[k][2]);
      acc[3] += (double)fmul_rn(st.w[k], st.z[k]);
      acc[4] += (double)st.w[k];
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    // wave_sum, written out: through the call the masked loss kernel
    // allocates one VGPR more
    double v = acc[i];
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) v += shfl_xor_d(v, k);
    out[i] = (float)v;
  }
}

// channel c of the ray's colour from ray_reduce's sums
CN_DEV float ray_colour(const float o[5], int c, int white_bg) {
  return white_bg ? fadd_rn(o[c] + 1.f, -o[4]) : o[c];
}

// Backward of one ray given d rgb_final (3) and d depth, as torch autograd.
// kAcc: g_acc, the gradient of the ray's weight sum (the silhouette term of
// the masked losses), is added to every sample's d weight as well; without it
// the sums are exactly the three below.
template <bool kAcc = false>
CN_DEV void ray_backward(const RayState& st, const float g[3], float gd, int white_bg,
                         float* dsig, float* drgb, float g_acc = 0.f) {
  const float gw_bg = white_bg ? -(g[0] + g[1] + g[2]) : 0.f;
  float dw[kMaxPer], wdT[kMaxPer];
  double part = 0.0;
#pragma unroll
  for (int k = 0; k < kMaxPer; ++k) {
    if (k < st.cnt) {
      // d weights = sum_c g_c c_c  + d(wsum) + gd * z
      float v = fadd_rn(fadd_rn(fmul_rn(g[0], st.c[k][0]), fmul_rn(g[1], st.c[k][1])), fmul_rn(g[2], st.c[k][2]));
      v = fadd_rn(v, gw_bg);
      if constexpr (kAcc) v = fadd_rn(v, g_acc);
      v = fadd_rn(v, fmul_rn(gd, st.z[k]));
      dw[k] = v;
      // grad of cumprod output T_k is dw_k * alpha_k; reversed cumsum of T_k * dT_k
      wdT[k] = fmul_rn(st.T[k], fmul_rn(v, st.alpha[k]));
      part += (double)wdT[k];
    }
  }
  // suffix sums strictly after each sample: across lanes, then within the lane
  double after = wave_exclusive_suffix_sum(part);
#pragma unroll
  for (int k = kMaxPer - 1; k >= 0; --k) {
    if (k < st.cnt) {
      const int s = st.n0 + k;
      // d trans_k = (sum_{j > k} T_j dT_j) / trans_k
      const float dtrans = (float)after / st.trans[k];
      after += (double)wdT[k];
      const float dalpha = fadd_rn(fmul_rn(dw[k], st.T[k]), -dtrans);
      dsig[s] = fmul_rn(fmul_rn(dalpha, st.e[k]), st.delta[k]);
      drgb[3 * s + 0] = fmul_rn(st.w[k], g[0]);
      drgb[3 * s + 1] = fmul_rn(st.w[k], g[1]);
      drgb[3 * s + 2] = fmul_rn(st.w[k], g[2]);
    }
  }
}

// ---------------------------------------------------------------- coarse + fine merge
// The planes of a coarse + fine ray kernel: sigma [R*N], rgb [R*N][3], z.
struct MergePlanes {
  const float *sig_c, *rgb_c, *zc;      // zc: [Nc] with zc_stride 0, else [R][Nc]
  int zc_stride, Nc;
  const float *sig_f, *rgb_f, *zf;      // zf: [R][Nf], ascending in every ray
  int Nf;
};
// One wave's LDS rows for the merged ray: kMaxRaySamples slots each (rgb x 3).
struct MergeRows {
  float *sig, *z, *rgb;
  int* src;                             // read only by merge_ray<true>
};

// The union of ray r's coarse and fine samples in z order, written to `m` for
// ray_forward.  A sample's merged position is its own index plus the number of
// the other list's samples before it; a coarse sample precedes a fine one at
// equal z (the coarse search counts zf < v, the fine one zc <= v), so with
// finite z the positions form a permutation of [0, Nc + Nf).
//
// Non-finite z (diverged weights): the two ranks need not form a permutation,
// so a slot may stay unwritten.  Such a slot is only ever read, from LDS, by
// ray_forward.  A kernel that later uses a slot's source as an index into
// global memory asks for the table m.src (kSrc): coarse i is i, fine j is
// Nc + j, and every slot starts as -1, "no source", which the kernel skips.
//
// zs: a kMaxRaySamples row that stages the ray's z, so that the rank searches'
// dependent reads cost LDS, not global-memory, latency.  It is dead after the
// call: the loss kernels pass their dsig row, which only the backward writes.
// place(p, fine, g): whatever else the kernel keeps per merged slot p, g being
// the sample's index in its own planes.
// Ends with the wave synchronised: every lane may read every row.
template <bool kSrc, class Place>
CN_DEV void merge_ray(const MergePlanes& a, int r, const MergeRows& m, float* zs, Place&& place) {
  const int lane = threadIdx.x & 63;
  const int Nc = a.Nc, Nf = a.Nf;
  const float* zcr = a.zc + (size_t)r * a.zc_stride;
  const float* zfr = a.zf + (size_t)r * Nf;
  if constexpr (kSrc)
    for (int p = lane; p < Nc + Nf; p += 64) m.src[p] = -1;
  for (int i = lane; i < Nc; i += 64) zs[i] = zcr[i];
  for (int j = lane; j < Nf; j += 64) zs[Nc + j] = zfr[j];
  wave_sync();
  for (int i = lane; i < Nc; i += 64) {
    const float v = zs[i];
    int lo = 0, hi = Nf;                    // count zf < v
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (zs[Nc + mid] < v) lo = mid + 1; else hi = mid; }
    const int p = i + lo;
    const size_t g = (size_t)r * Nc + i;
    m.sig[p] = a.sig_c[g];
    m.z[p] = v;
    m.rgb[3 * p + 0] = a.rgb_c[3 * g + 0];
    m.rgb[3 * p + 1] = a.rgb_c[3 * g + 1];
    m.rgb[3 * p + 2] = a.rgb_c[3 * g + 2];
    if constexpr (kSrc) m.src[p] = i;
    place(p, false, g);
  }
  for (int j = lane; j < Nf; j += 64) {
    const float v = zs[Nc + j];
    int lo = 0, hi = Nc;                    // count zc <= v
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (zs[mid] <= v) lo = mid + 1; else hi = mid; }
    const int p = j + lo;
    const size_t g = (size_t)r * Nf + j;
    m.sig[p] = a.sig_f[g];
    m.z[p] = v;
    m.rgb[3 * p + 0] = a.rgb_f[3 * g + 0];
    m.rgb[3 * p + 1] = a.rgb_f[3 * g + 1];
    m.rgb[3 * p + 2] = a.rgb_f[3 * g + 2];
    if constexpr (kSrc) m.src[p] = Nc + j;
    place(p, true, g);
  }
  wave_sync();
}
template <bool kSrc>
CN_DEV void merge_ray(const MergePlanes& a, int r, const MergeRows& m, float* zs) {
  merge_ray<kSrc>(a, r, m, zs, [](int, bool, size_t) {});
}

// rgb, expected depth and (out_acc given) opacity of ray r from ray_reduce's
// sums: the forward kernels' lane-0 stores
CN_DEV void store_ray(const float o[5], int r, int white_bg, float* out_rgb, float* out_depth, float* out_acc) {
  if ((threadIdx.x & 63) != 0) return;
  for (int c = 0; c < 3; ++c) out_rgb[3 * r + c] = ray_colour(o, c, white_bg);
  out_depth[r] = o[3];
  if (out_acc) out_acc[r] = o[4];
}

}  // namespace cn
