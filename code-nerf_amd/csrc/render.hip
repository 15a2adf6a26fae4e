// Ray generation, alpha compositing (+ backward) and the image loss.
//
//   get_rays            reference src/utils.py:10-19
//   composite fwd/bwd   reference src/utils.py:34-47 and its autograd
//   render_loss         composite + chunk-mean MSE (src/trainer.py:75) + the
//                       composite backward, fused per ray for training
//   render_loss<true>   the same with a weight per ray and a silhouette term
//                       on the ray's accumulated opacity (no reference
//                       counterpart in code)
//
// The ray itself (one wave per ray: ray_forward, ray_reduce, ray_backward and
// the coarse + fine merge_ray) is cn_ray.h.
#include "cn_ray.h"

namespace cn {

// ---------------------------------------------------------------- rays
__global__ __launch_bounds__(256) void get_rays_kernel(int H, int W, double focal, int focal_f64,
                                                       const float* __restrict__ c2w,
                                                       float* __restrict__ ro, float* __restrict__ vd) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int row = p / W, col = p - row * W;
  float dx, dy;
  if (focal_f64) {   // (i - W/2) / focal formed in float64, then cast (type promotion)
    dx = (float)(((double)col - W * 0.5) / focal);
    dy = (float)(-(((double)row - H * 0.5) / focal));
  } else {
    const float f = (float)focal;
    dx = ((float)col - W * 0.5f) / f;
    dy = -(((float)row - H * 0.5f) / f);
  }
  float d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    // sum_b dirs[b] * c2w[a][b], summed in order, no fma
    float s = fmul_rn(dx, c2w[4 * a + 0]);
    s = fadd_rn(s, fmul_rn(dy, c2w[4 * a + 1]));
    s = fadd_rn(s, fmul_rn(-1.f, c2w[4 * a + 2]));
    d[a] = s;
  }
  // torch.norm(dim=-1) of a float32 3-vector on the CPU (src/utils.py:16):
  // sqrt(fma(d2, d2, fma(d1, d1, d0 * d0))) -- matched bit for bit against
  // torch 2.10's CPU kernel over 2e5 random vectors
  const float nrm = sqrtf(__builtin_fmaf(d[2], d[2], __builtin_fmaf(d[1], d[1], fmul_rn(d[0], d[0]))));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    vd[3 * p + a] = d[a] / nrm;
    ro[3 * p + a] = c2w[4 * a + 3];
  }
}

// Autograd of get_rays with respect to c2w (no reference counterpart: the
// reference never differentiates through the camera).  With cam = (dx, dy, -1),
// d = R cam, v = d / |d|:
//   g = (d_v - v (v . d_v)) / |d|,  dR[a][b] = sum_rays g_a cam_b,
//   d c2w[a][3] = sum_rays d_rays_o_a.
// d and |d| are the forward's float values; everything after them, and both
// stages of the sum, in float64.  Stage 1: one partial (12 doubles, the 3 x 4
// row-major layout of the output) per 256-pixel block, summed by a fixed
// butterfly and a fixed order over the block's waves; stage 2: one block sums
// the partials in a fixed order.  Written, not accumulated; deterministic.
constexpr int kRaysBwdBlock = 256;

__global__ __launch_bounds__(kRaysBwdBlock) void get_rays_bwd_partial_kernel(
    int H, int W, double focal, int focal_f64, const float* __restrict__ c2w, const float* __restrict__ dro,
    const float* __restrict__ dvd, double* __restrict__ part) {
  __shared__ double red[kRaysBwdBlock / 64][12];
  const int p = blockIdx.x * kRaysBwdBlock + threadIdx.x;
  double t[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) t[i] = 0.0;
  if (p < H * W) {
    const int row = p / W, col = p - row * W;
    float cam[3];
    if (focal_f64) {
      cam[0] = (float)(((double)col - W * 0.5) / focal);
      cam[1] = (float)(-(((double)row - H * 0.5) / focal));
    } else {
      const float f = (float)focal;
      cam[0] = ((float)col - W * 0.5f) / f;
      cam[1] = -(((float)row - H * 0.5f) / f);
    }
    cam[2] = -1.f;
    float d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float s = fmul_rn(cam[0], c2w[4 * a + 0]);
      s = fadd_rn(s, fmul_rn(cam[1], c2w[4 * a + 1]));
      s = fadd_rn(s, fmul_rn(-1.f, c2w[4 * a + 2]));
      d[a] = s;
    }
    const double nrm = (double)sqrtf(__builtin_fmaf(d[2], d[2], __builtin_fmaf(d[1], d[1], fmul_rn(d[0], d[0]))));
    double v[3], gv[3], dot = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[a] = (double)d[a] / nrm;
      gv[a] = (double)dvd[3 * p + a];
      dot += v[a] * gv[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double g = (gv[a] - v[a] * dot) / nrm;
#pragma unroll
      for (int b = 0; b < 3; ++b) t[4 * a + b] = g * (double)cam[b];
      t[4 * a + 3] = (double)dro[3 * p + a];
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const double s = wave_sum(t[i]);
    if (lane == 0) red[w][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < 12) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kRaysBwdBlock / 64; ++k) s += red[k][threadIdx.x];
    part[(size_t)blockIdx.x * 12 + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(kRaysBwdBlock) void get_rays_bwd_final_kernel(const double* __restrict__ part,
                                                                           int nblocks, float* __restrict__ dc2w) {
  __shared__ double red[kRaysBwdBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = 0; i < 12; ++i) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kRaysBwdBlock) s += part[(size_t)b * 12 + i];
    s = wave_sum(s);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      double tot = 0.0;
#pragma unroll
      for (int k = 0; k < kRaysBwdBlock / 64; ++k) tot += red[k];
      dc2w[i] = (float)tot;
    }
    __syncthreads();
  }
}

// rgb_out (R,3), depth (R): volume_rendering forward
__global__ __launch_bounds__(256) void composite_fwd_kernel(const float* __restrict__ sig, const float* __restrict__ rgb,
                                                            const float* __restrict__ z, int z_stride, int R, int N,
                                                            int white_bg, float* __restrict__ out_rgb,
                                                            float* __restrict__ out_depth, float* __restrict__ out_w) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  RayState st;
  ray_forward(st, sig + (size_t)r * N, rgb + (size_t)r * N * 3, z + (size_t)r * z_stride, N);
  float o[5];
  ray_reduce(st, o);
  store_ray(o, r, white_bg, out_rgb, out_depth, nullptr);
  if (out_w) {
#pragma unroll
    for (int k = 0; k < kMaxPer; ++k)
      if (k < st.cnt) out_w[(size_t)r * N + st.n0 + k] = st.w[k];
  }
}

__global__ __launch_bounds__(256) void composite_bwd_kernel(const float* __restrict__ sig, const float* __restrict__ rgb,
                                                            const float* __restrict__ z, int z_stride, int R, int N,
                                                            int white_bg, const float* __restrict__ g_rgb,
                                                            const float* __restrict__ g_depth,
                                                            float* __restrict__ dsig, float* __restrict__ drgb) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  RayState st;
  ray_forward(st, sig + (size_t)r * N, rgb + (size_t)r * N * 3, z + (size_t)r * z_stride, N);
  const float g[3] = {g_rgb[3 * r], g_rgb[3 * r + 1], g_rgb[3 * r + 2]};
  const float gd = g_depth ? g_depth[r] : 0.f;
  ray_backward(st, g, gd, white_bg, dsig + (size_t)r * N, drgb + (size_t)r * N * 3);
}

// The kMasked instantiation of both loss kernels: a weight m_r >= 0 per ray (NULL:
// 1), and with sil_coef > 0 a target a_r for the ray's accumulated opacity
// acc_r = sum_k w_k (ray_reduce's o[4]; the fine kernel's runs over the merged
// samples).  Per chunk of nb rays
//   loss = sum_r [ m_r sum_c (col_rc - gt_rc)^2 + 3 sil_coef (acc_r - a_r)^2 ] / (3 nb)
// so ray_se[r] = m_r se_r + 3 sil_coef (acc_r - a_r)^2 goes through
// chunk_loss_kernel unchanged, d col_c = m_r (2 / (3 nb)) diff_c, and
// d acc = sil_coef (2 / nb) (acc_r - a_r) joins every sample's d weight in
// ray_backward.  m = 1 and sil_coef = 0 give the plain kernels' bits: every
// other operation is ray_loss's, shared with them.  The host passes
// sil_coef = 0 when acc_target is NULL.
struct RayMask {
  const float* weight;       // [R] or NULL
  const float* acc_target;   // [R]; read only when sil_coef > 0
  float sil_coef;
  float* out_acc;            // [R] or NULL
};

// ray_se and the gradient of the weight sum of one masked ray; g (already
// (2 / (3 nb)) diff) is scaled by the ray's weight in place
CN_DEV float masked_ray_loss(const RayMask& mk, int r, int nb, float se, float acc, float g[3], float* g_acc) {
  const float m = mk.weight ? mk.weight[r] : 1.f;
  for (int c = 0; c < 3; ++c) g[c] = fmul_rn(m, g[c]);
  float out = fmul_rn(m, se);
  *g_acc = 0.f;
  if (mk.sil_coef > 0.f) {
    const float d = fadd_rn(acc, -mk.acc_target[r]);
    out = fadd_rn(out, fmul_rn(fmul_rn(3.f, mk.sil_coef), fmul_rn(d, d)));
    *g_acc = fmul_rn(fmul_rn(mk.sil_coef, 2.f / (float)nb), d);
  }
  return out;
}

// The loss body of the four loss kernels, from ray_reduce's sums o of ray r:
// the ray's colour, its squared error and g = d loss / d colour of the
// chunk-mean MSE (chunk = `chunk` consecutive rays, src/trainer.py:69,75);
// lane 0 stores out_rgb and ray_se.  kMasked adds the loss of RayMask
// (masked_ray_loss) and the opacity output; the plain instantiation does not
// read mk.  -> d loss / d opacity (0 when not masked), for ray_backward.
template <bool kMasked>
CN_DEV float ray_loss(const float o[5], int r, int R, int white_bg, const float* gt, int chunk, float* out_rgb,
                      float* ray_se, const RayMask& mk, float g[3]) {
  float col[3];
  const int c0 = (r / chunk) * chunk;
  const int nb = min(chunk, R - c0);
  const float inv = 1.f / (float)(3 * nb);
  float se = 0.f;
  for (int c = 0; c < 3; ++c) {
    col[c] = ray_colour(o, c, white_bg);
    const float diff = col[c] - gt[3 * r + c];
    se += diff * diff;
    // d mean(diff^2) = 2 * diff / numel
    g[c] = fmul_rn(fmul_rn(inv, 2.f), diff);
  }
  float g_acc = 0.f;
  if constexpr (kMasked) se = masked_ray_loss(mk, r, nb, se, o[4], g, &g_acc);
  if ((threadIdx.x & 63) == 0) {
    for (int c = 0; c < 3; ++c) out_rgb[3 * r + c] = col[c];
    ray_se[r] = se;
    if constexpr (kMasked)
      if (mk.out_acc) mk.out_acc[r] = o[4];
  }
  return g_acc;
}

// Training: composite, the loss (ray_loss), composite backward.
template <bool kMasked>
__global__ __launch_bounds__(256) void render_loss_kernel(const float* __restrict__ sig, const float* __restrict__ rgb,
                                                          const float* __restrict__ z, int z_stride, int R, int N,
                                                          int white_bg, const float* __restrict__ gt, int chunk,
                                                          float* __restrict__ out_rgb, float* __restrict__ ray_se,
                                                          float* __restrict__ dsig, float* __restrict__ drgb,
                                                          RayMask mk) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  RayState st;
  ray_forward(st, sig + (size_t)r * N, rgb + (size_t)r * N * 3, z + (size_t)r * z_stride, N);
  float o[5], g[3];
  ray_reduce(st, o);
  const float g_acc = ray_loss<kMasked>(o, r, R, white_bg, gt, chunk, out_rgb, ray_se, mk, g);
  ray_backward<kMasked>(st, g, 0.f, white_bg, dsig + (size_t)r * N, drgb + (size_t)r * N * 3, g_acc);
}

// chunk-mean MSE values from per-ray squared errors (one block per chunk)
__global__ __launch_bounds__(256) void chunk_loss_kernel(const float* __restrict__ ray_se, int R, int chunk,
                                                         float* __restrict__ loss) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  const int a = c * chunk, b = min(R, a + chunk);
  double s = 0.0;
  for (int r = a + threadIdx.x; r < b; r += 256) s += ray_se[r];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[c] = (float)(red[0] / (3.0 * (b - a)));
}

// ---------------------------------------------------------------- fine pass
// Hierarchical ("coarse + fine") sampling: the BASELINE configs' 64 + 64
// samples.  The reference has no fine pass, so this
// follows NeRF's sample_pdf with the CodeNeRF MLP shared by both passes;
// oracle: oracle/ref_cpu.py sample_pdf / fine_render_loss (parity unpinned).

// Importance samples of one ray per wave: bins = midpoints of the coarse z,
// pdf = (w[1:-1] + 1e-5) / sum, cdf = [0, cumsum] (float64, rounded once),
// u_j = (j + rnd_j) / Nf (stratified, so z_f comes out sorted), z_f = inverse
// cdf with NeRF's degenerate-bin rule (denom < 1e-5 -> 1).
__global__ __launch_bounds__(256) void sample_pdf_kernel(const float* __restrict__ sig, const float* __restrict__ z,
                                                         int z_stride, int R, int Nc,
                                                         const float* __restrict__ rnd, int Nf,
                                                         float* __restrict__ zf) {
  __shared__ float cdf_s[4][kMaxRaySamples], bin_s[4][kMaxRaySamples];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wv;
  if (r >= R) return;                       // wave-uniform; no block barriers below
  const float* zr = z + (size_t)r * z_stride;
  RayState st;
  ray_forward(st, sig + (size_t)r * Nc, nullptr, zr, Nc);
  // interior weights s = 1 .. Nc-2, +1e-5 (float, as torch: weights + 1e-5)
  float wv_[kMaxPer];
  double part = 0.0;
#pragma unroll
  for (int k = 0; k < kMaxPer; ++k) {
    const int s = st.n0 + k;
    wv_[k] = 0.f;
    if (k < st.cnt && s >= 1 && s <= Nc - 2) {
      wv_[k] = st.w[k] + 1e-5f;
      part += (double)wv_[k];
    }
  }
  const double incl = wave_inclusive_sum(part);
  const double total = __hiloint2double(__shfl(__double2hiint(incl), 63), __shfl(__double2loint(incl), 63));
  double run = incl - part;             // exclusive prefix over lanes
  float* cdf = cdf_s[wv];
  float* bins = bin_s[wv];
#pragma unroll
  for (int k = 0; k < kMaxPer; ++k) {
    const int s = st.n0 + k;
    if (k < st.cnt) {
      run += (double)wv_[k];
      // cdf[i] = sum_{s=1..i} / total for i = 1 .. Nc-2; cdf[0] = 0
      if (s >= 1 && s <= Nc - 2) cdf[s] = (float)(run / total);
      if (s == 0) cdf[0] = 0.f;
      if (s + 1 < Nc) bins[s] = fmul_rn(0.5f, fadd_rn(zr[s], zr[s + 1]));
    }
  }
  wave_sync();
  const int nb = Nc - 1;                   // cdf / bin entries
  for (int j = lane; j < Nf; j += 64) {
    const float u = (float)j + rnd[(size_t)r * Nf + j];
    const float uu = u / (float)Nf;
    // searchsorted(cdf, uu, right=True): first index with cdf > uu
    int lo = 0, hi = nb;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] <= uu) lo = mid + 1; else hi = mid;
    }
    const int below = max(0, lo - 1), above = min(nb - 1, lo);
    const float cb = cdf[below], ca = cdf[above];
    const float bb = bins[below], ba = bins[above];
    float denom = fadd_rn(ca, -cb);
    if (denom < 1e-5f) denom = 1.f;
    const float t = fadd_rn(uu, -cb) / denom;
    zf[(size_t)r * Nf + j] = fadd_rn(bb, fmul_rn(t, fadd_rn(ba, -bb)));
  }
}

// Fine composite + the loss (ray_loss) + backward over the union of the coarse
// and fine samples of each ray (merge_ray).  dsig_c / drgb_c are ACCUMULATED
// into (they already hold the coarse loss's gradient); dsig_f / drgb_f are
// written.  With kMasked the opacity runs over the merged samples.
template <bool kMasked>
__global__ __launch_bounds__(256) void fine_render_loss_kernel(
    const float* __restrict__ sig_c, const float* __restrict__ rgb_c, const float* __restrict__ zc, int zc_stride,
    int Nc, const float* __restrict__ sig_f, const float* __restrict__ rgb_f, const float* __restrict__ zf, int Nf,
    int R, int white_bg, const float* __restrict__ gt, int chunk, float* __restrict__ out_rgb,
    float* __restrict__ ray_se, float* __restrict__ dsig_c, float* __restrict__ drgb_c,
    float* __restrict__ dsig_f, float* __restrict__ drgb_f, RayMask mk) {
  __shared__ float m_sig[4][kMaxRaySamples], m_z[4][kMaxRaySamples], m_rgb[4][kMaxRaySamples * 3];
  __shared__ float m_dsig[4][kMaxRaySamples], m_drgb[4][kMaxRaySamples * 3];
  __shared__ int m_src[4][kMaxRaySamples];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wv;
  if (r >= R) return;                       // wave-uniform; only wave-level sync below
  const int N = Nc + Nf;
  // the gradients scatter through m_src; m_dsig stages z until the backward
  merge_ray<true>(MergePlanes{sig_c, rgb_c, zc, zc_stride, Nc, sig_f, rgb_f, zf, Nf}, r,
                  MergeRows{m_sig[wv], m_z[wv], m_rgb[wv], m_src[wv]}, m_dsig[wv]);
  RayState st;
  ray_forward(st, m_sig[wv], m_rgb[wv], m_z[wv], N);
  float o[5], g[3];
  ray_reduce(st, o);
  const float g_acc = ray_loss<kMasked>(o, r, R, white_bg, gt, chunk, out_rgb, ray_se, mk, g);
  ray_backward<kMasked>(st, g, 0.f, white_bg, m_dsig[wv], m_drgb[wv], g_acc);
  wave_sync();
  for (int p = lane; p < N; p += 64) {
    const int src = m_src[wv][p];
    if (src < 0) continue;
    if (src < Nc) {
      const size_t g = (size_t)r * Nc + src;
      dsig_c[g] += m_dsig[wv][p];
      for (int c = 0; c < 3; ++c) drgb_c[3 * g + c] += m_drgb[wv][3 * p + c];
    } else {
      const size_t g = (size_t)r * Nf + (src - Nc);
      dsig_f[g] = m_dsig[wv][p];
      for (int c = 0; c < 3; ++c) drgb_f[3 * g + c] = m_drgb[wv][3 * p + c];
    }
  }
}

// Forward half of fine_render_loss_kernel (test-time rendering): the same
// merge, ray_forward and ray_reduce, so the rgb comes out bit for bit as the
// loss kernel's; plus depth and, when out_acc is given, the weight sum.  No
// gt, no gradients, no source table.
__global__ __launch_bounds__(256) void composite_fine_fwd_kernel(
    const float* __restrict__ sig_c, const float* __restrict__ rgb_c, const float* __restrict__ zc, int zc_stride,
    int Nc, const float* __restrict__ sig_f, const float* __restrict__ rgb_f, const float* __restrict__ zf, int Nf,
    int R, int white_bg, float* __restrict__ out_rgb, float* __restrict__ out_depth, float* __restrict__ out_acc) {
  __shared__ float m_sig[4][kMaxRaySamples], m_z[4][kMaxRaySamples], m_rgb[4][kMaxRaySamples * 3];
  __shared__ float z_stage[4][kMaxRaySamples];
  const int wv = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wv;
  if (r >= R) return;                       // wave-uniform; only wave-level sync below
  merge_ray<false>(MergePlanes{sig_c, rgb_c, zc, zc_stride, Nc, sig_f, rgb_f, zf, Nf}, r,
                   MergeRows{m_sig[wv], m_z[wv], m_rgb[wv], nullptr}, z_stage[wv]);
  RayState st;
  ray_forward(st, m_sig[wv], m_rgb[wv], m_z[wv], Nc + Nf);
  float o[5];
  ray_reduce(st, o);
  store_ray(o, r, white_bg, out_rgb, out_depth, out_acc);
}

// ---------------------------------------------------------------- misc
__global__ __launch_bounds__(256) void stratified_points_kernel(const float* __restrict__ ro, const float* __restrict__ vd,
                                                                const float* __restrict__ z, int z_stride, int R, int N,
                                                                float* __restrict__ xyz, float* __restrict__ vrep) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= R * N) return;
  const int r = m / N, s = m - r * N;
  const float zz = z[(size_t)r * z_stride + s];
  for (int a = 0; a < 3; ++a) {
    const float d = vd[3 * r + a];
    xyz[3 * m + a] = fadd_rn(ro[3 * r + a], fmul_rn(d, zz));
    vrep[3 * m + a] = d;
  }
}

}  // namespace cn
