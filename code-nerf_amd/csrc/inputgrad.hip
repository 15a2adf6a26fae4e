// Gradient of the network with respect to its per-sample inputs (position and
// view direction) and, per ray, with respect to the ray origin and direction.
// No reference counterpart: the reference never differentiates through the
// camera ("Pose Optimizing" is an open item there); the arithmetic is the
// autograd of src/model.py:4-7,38,47 restated.
//
// The dX chain ends at dA of the first layer.  What is left of the backward is
//
//   dPE [63] = W_xyz^T          . dA_0           (dA of encoding_xyz, 256 wide)
//   dDir[27] = W_vd[:,256:283]^T . dA_vd[:256]    (dA of encoding_viewdir)
//   dxyz_c  = dPE[c]  + sum_i 2^i (cos(2^i x_c) dPE[3+3i+c]  - sin(2^i x_c) dPE[33+3i+c]),  i < 10
//   dvdir_c = dDir[c] + sum_i 2^i (cos(2^i v_c) dDir[3+3i+c] - sin(2^i v_c) dDir[15+3i+c]), i < 4
//
// in the chain kernels' orientation: a wave owns a 32-sample slab and computes
// dPE^T[64 slots][32 samples] = W^T . dA^T (two output tiles) and dDir^T (one)
// over K = 256.  The stored dA slab IS the packed B operand: the plane layout
// (cn_layout.h) keeps, per lane, the 16 bytes an MFMA lane holds after the
// chain's epilogue -- 8 bf16 in bf16_acc_feature order, or 4 fp32 that are 4
// k-steps of v_mfma_f32_32x32x2_f32 in f32_acc_feature order -- so one 16-B
// load per lane is a B fragment with no transposition.
//
// The A operand comes from the fp32 parameter tensors, converted once per
// workgroup into LDS in the matching k order (96 blocks of 1 KiB): bf16 planes
// multiply the weight as a bf16 hi + lo pair (two MFMAs per block; the stored
// gradient is the only rounded operand), fp32 planes the fp32 weight.
//
// Output rows are laid out so that a lane half owns the sin and the cos slot
// of one argument (pe_slot_feature / dir_slot_feature): accumulator register r
// of tile T on lane half h is slot 16 T + r of that half.  x, v and the
// sin / cos are recomputed in fp32 registers from the inputs with the correctly
// rounded sincosf of the fp32 forward (the factor 2^9 multiplies any error of
// the argument reduction); the two lane halves of a sample are combined in-wave.
#pragma once
#include "cn_common.h"
#include "cn_layout.h"
#include "cn_ray.h"

namespace cn {

constexpr int kIgWaves = 4;
constexpr int kIgBlocks = 96;                       // A-fragment blocks of 1 KiB in LDS
constexpr int kIgLdsBytes = kIgBlocks * kBlockBytes;
constexpr int kIgMaxWorkgroups = 256;               // persistent: one per CU (96 KiB of LDS each)

struct InputGradArgs {
  const float* const* params;   // reference state_dict order
  int w_vd;                     // index of encoding_viewdir.0.weight ([256][283]); encoding_xyz.0.weight is 0
  const void* dA0;              // dA plane of encoding_xyz, width 256, at the launch's first row
  const void* dAv;              // dA plane of encoding_viewdir, width 288 (256 feature columns read)
  int M, Mp;
  int mode;                     // 0: explicit points, 1: rays x samples (as ChainArgs)
  int nsamp, z_stride;
  const float *xyz, *vdir, *rays_o, *rays_d, *zvals;
  float* dxyz;                  // [Mp][3]
  float* dvdir;                 // [Mp][3]
};

// output row n of tile T (0, 1: dPE; 2: dDir) -> reference input feature (-1: pad)
CN_DEV int ig_row_feature(int T, int n) {
  const int hh = (n >> 2) & 1, r = (n & 3) + 4 * (n >> 3);     // inverse of acc_row
  return T < 2 ? pe_slot_feature(hh, 16 * T + r) : dir_slot_feature(hh, r);
}

template <bool BF16>
__global__ __launch_bounds__(kIgWaves * 64) void input_grad_kernel(InputGradArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[kIgLdsBytes];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int s = lane & 31, h = lane >> 5;

  // ---- stage W^T as A fragments.  bf16: block ((T * 16 + q) * 2 + part), lane
  // (n, h): 8 elements W[bf16_acc_feature(q, h, j)][row feature], part 0 = hi,
  // 1 = lo.  fp32: block (T * 32 + qq), 4 elements W[8 qq + 4 h + i][row feature]
  // (= f32_acc_feature(4 qq + i, h)).
  {
    const float* wx = a.params[0];
    const float* wv = a.params[a.w_vd];
    for (int it = threadIdx.x; it < kIgBlocks * 64; it += kIgWaves * 64) {
      const int b = it >> 6, l = it & 63;
      const int n = l & 31, hh = l >> 5;
      const int T = b >> 5;
      const int feat = ig_row_feature(T, n);
      const float* col = T < 2 ? wx + feat : wv + 256 + feat;
      const int stride = T < 2 ? 63 : 283;
      if constexpr (BF16) {
        const int q = (b & 31) >> 1, part = b & 1;
        uint32_t pk[4];
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
          uint32_t word = 0u;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int f = bf16_acc_feature(q, hh, 2 * jp + e);
            const float v = feat >= 0 ? col[f * stride] : 0.f;
            const __bf16 hi = (__bf16)v;
            const __bf16 o = part ? (__bf16)(v - (float)hi) : hi;
            word |= (uint32_t)__builtin_bit_cast(uint16_t, o) << (16 * e);
          }
          pk[jp] = word;
        }
        *(u32x4*)(smem + b * kBlockBytes + l * 16) = u32x4{pk[0], pk[1], pk[2], pk[3]};
      } else {
        const int qq = b & 31;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = feat >= 0 ? col[(8 * qq + 4 * hh + i) * stride] : 0.f;
        *(f32x4*)(smem + b * kBlockBytes + l * 16) = f32x4{v[0], v[1], v[2], v[3]};
      }
    }
  }
  __syncthreads();

  constexpr int ES = BF16 ? 2 : 4;
  const int nslab = a.Mp >> 5;
  for (int slab = blockIdx.x * kIgWaves + w; slab < nslab; slab += gridDim.x * kIgWaves) {
    const char* p0 = (const char*)a.dA0 + (size_t)slab * 256u * 32u * ES;
    const char* pv = (const char*)a.dAv + (size_t)slab * 288u * 32u * ES;
    f32x16 acc0 = {}, acc1 = {}, acc2 = {};
    if constexpr (BF16) {
      // (not fully unrolled: the compiler would hoist all 96 fragment reads
      // above the first MFMA and spill)
#pragma unroll 2
      for (int q = 0; q < 16; ++q) {
        const int off = slab_off(s, 16 * q + 4 * h, 2);
        const bf16x8 b0 = __builtin_bit_cast(bf16x8, *(const u32x4*)(p0 + off));
        const bf16x8 bv = __builtin_bit_cast(bf16x8, *(const u32x4*)(pv + off));
        auto frag = [&](int T, int part) {
          return __builtin_bit_cast(bf16x8, *(const u32x4*)(smem + ((T * 16 + q) * 2 + part) * kBlockBytes + lane * 16));
        };
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(0, 0), b0, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(0, 1), b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(1, 0), b0, acc1, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(1, 1), b0, acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(2, 0), bv, acc2, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(2, 1), bv, acc2, 0, 0, 0);
      }
    } else {
#pragma unroll 4
      for (int qq = 0; qq < 32; ++qq) {
        const int off = slab_off(s, 8 * qq + 4 * h, 4);
        const f32x4 b0 = *(const f32x4*)(p0 + off);
        const f32x4 bv = *(const f32x4*)(pv + off);
        const f32x4 a0 = *(const f32x4*)(smem + (0 * 32 + qq) * kBlockBytes + lane * 16);
        const f32x4 a1 = *(const f32x4*)(smem + (1 * 32 + qq) * kBlockBytes + lane * 16);
        const f32x4 a2 = *(const f32x4*)(smem + (2 * 32 + qq) * kBlockBytes + lane * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i], b0[i], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[i], b0[i], acc1, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[i], bv[i], acc2, 0, 0, 0);
        }
      }
    }

    // ---- this lane's sample: inputs as the chain prologue forms them
    const int m = slab * 32 + s;
    const bool valid = m < a.M;
    const int mc = valid ? m : a.M - 1;
    float x[3], v[3];
    if (a.mode == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { x[k] = a.xyz[3 * mc + k]; v[k] = a.vdir[3 * mc + k]; }
    } else {
      const int r = mc / a.nsamp;
      const int si = mc - r * a.nsamp;
      const float z = a.zvals[r * a.z_stride + si];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v[k] = a.rays_d[3 * r + k];
        x[k] = fadd_rn(a.rays_o[3 * r + k], fmul_rn(v[k], z));     // src/utils.py:30, no fma
      }
    }

    // ---- through the positional encodings.  Lane half h holds slots
    // (raw, raw, sin a_k, cos a_k, ...) of arguments p = 15 h + k (PE) and
    // p = k on half 0, 7 + k on half 1 (dir): component p % 3, octave p / 3.
    float pe[32];
#pragma unroll
    for (int i = 0; i < 16; ++i) { pe[i] = acc0[i]; pe[16 + i] = acc1[i]; }
    float dx[3] = {0.f, 0.f, 0.f}, dv[3] = {0.f, 0.f, 0.f};
    if (h == 0) { dx[0] = pe[0]; dx[1] = pe[1]; dv[0] = acc2[0]; dv[1] = acc2[1]; }
    else { dx[2] = pe[0]; dv[2] = acc2[0]; }
#pragma unroll
    for (int k = 0; k < 15; ++k) {
      const int comp = k % 3;                                   // (15 h + k) % 3
      const float scale = (float)(1 << (k / 3)) * (h ? 32.f : 1.f);   // 2^(5 h + k / 3)
      float sn, cs;
      sincosf(x[comp] * scale, &sn, &cs);
      dx[comp] += scale * (cs * pe[2 + 2 * k] - sn * pe[3 + 2 * k]);
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const int c0 = k % 3, c1 = (7 + k) % 3;
      const float scale = h ? (float)(1 << ((7 + k) / 3)) : (float)(1 << (k / 3));
      const float arg = h ? v[c1] : v[c0];
      float sn, cs;
      sincosf(arg * scale, &sn, &cs);
      float c = scale * (cs * acc2[2 + 2 * k] - sn * acc2[3 + 2 * k]);
      if (h && k >= 5) c = 0.f;                                  // half 1 holds arguments 7..11 only
      const int comp = h ? c1 : c0;
#pragma unroll
      for (int j = 0; j < 3; ++j) dv[j] += comp == j ? c : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      dx[j] += __shfl_xor(dx[j], 32);
      dv[j] += __shfl_xor(dv[j], 32);
    }
    // rows >= M of the pad are written as 0; half 0 stores d_xyz, half 1 d_viewdir
    float* out = h ? a.dvdir : a.dxyz;
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * (size_t)m + j] = valid ? (h ? dv[j] : dx[j]) : 0.f;
  }
}

// Per-ray sums (mode B), one wave per ray like the compositing kernels:
//   d_rays_o[r] = sum_s d_xyz,  d_rays_d[r] = sum_s (z_s d_xyz + d_viewdir)
// lane l adds samples l, l + 64, ... in order, then a fixed xor butterfly; all
// in float64, no atomics: the result does not depend on the launch.
__global__ __launch_bounds__(256) void ray_grad_kernel(const float* __restrict__ dxyz,
                                                       const float* __restrict__ dvdir,
                                                       const float* __restrict__ z, int z_stride, int R, int N,
                                                       float* __restrict__ dro, float* __restrict__ drd) {
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (ray >= R) return;
  double so[3] = {0.0, 0.0, 0.0}, sd[3] = {0.0, 0.0, 0.0};
  for (int si = lane; si < N; si += 64) {
    const size_t m = (size_t)ray * N + si;
    const double zs = (double)z[(size_t)ray * z_stride + si];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double g = (double)dxyz[3 * m + c];
      so[c] += g;
      sd[c] += zs * g + (double)dvdir[3 * m + c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    so[c] = wave_sum(so[c]);
    sd[c] = wave_sum(sd[c]);
  }
  if (lane < 3) {
    dro[3 * (size_t)ray + lane] = (float)(lane == 0 ? so[0] : lane == 1 ? so[1] : so[2]);
    drd[3 * (size_t)ray + lane] = (float)(lane == 0 ? sd[0] : lane == 1 ? sd[1] : sd[2]);
  }
}

}  // namespace cn
