// Iso-surface extraction: marching tetrahedra on the Kuhn triangulation of a
// lattice of densities.  No reference counterpart; include/codenerf.h and
// DESIGN.md 8.5 have the definition.
//
// Lattice point (ix, iy, iz) is c = (ix ny + iy) nz + iz and is INSIDE iff
// !(field[c] < iso) (NaN inside).  It owns up to 7 edges, edge k towards the
// offset code m = k + 1 (x = bit 2, y = bit 1, z = bit 0); a crossing edge (one
// end inside) carries one vertex, row voff[c] + popcount(vflags[c] below bit k).
// The cube with lowest corner c is cut into the 6 tetrahedra of mesh_tables.h;
// its triangles are rows toff[c] ... in tetrahedron, then table order.
//
// One thread per lattice point, iz fastest, so the field reads of a wave are
// contiguous; the 7 neighbour values come from cache.  Two passes around the
// caller's prefix sums, as the sparse path.  No atomics; every output element
// is written by exactly one thread.
#include "cn_common.h"
#include "mesh_tables.h"

namespace cn {

struct MeshDims {
  int nx, ny, nz;
};

// Bit m of the result: the corner at offset code m exists and is inside; bit
// 8 + m: it exists.  val[m]: its field value (0 where it does not exist).
CN_DEV uint32_t mesh_corners(const float* __restrict__ field, MeshDims d, int c, int ix, int iy, int iz, float iso,
                             float val[8]) {
  uint32_t bits = 0;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int dx = (m >> 2) & 1, dy = (m >> 1) & 1, dz = m & 1;
    const bool ok = ix + dx < d.nx && iy + dy < d.ny && iz + dz < d.nz;
    val[m] = 0.f;
    if (ok) {
      val[m] = field[c + (dx * d.ny + dy) * d.nz + dz];
      bits |= (0x100u | (uint32_t)!(val[m] < iso)) << m;
    }
  }
  return bits;
}

// the crossing owned edges of the point whose corner bits are `bits`
CN_DEV uint32_t mesh_vflags(uint32_t bits) {
  const uint32_t in0 = bits & 1u;
  uint32_t f = 0;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const int m = k + 1;
    if (((bits >> (8 + m)) & 1u) && (((bits >> m) & 1u) != in0)) f |= 1u << k;
  }
  return f;
}

// inside mask of tetrahedron t (local vertices v0 .. v3) from the cube's corner bits
CN_DEV uint32_t mesh_tet_mask(uint32_t bits, int t) {
  // v1 / v2 offset codes of the 6 axis permutations in lexicographic order
  constexpr uint32_t kV1 = 4u | 4u << 3 | 2u << 6 | 2u << 9 | 1u << 12 | 1u << 15;
  constexpr uint32_t kV2 = 6u | 5u << 3 | 6u << 6 | 3u << 9 | 5u << 12 | 3u << 15;
  const uint32_t v1 = (kV1 >> (3 * t)) & 7u, v2 = (kV2 >> (3 * t)) & 7u;
  return (bits & 1u) | ((bits >> v1) & 1u) << 1 | ((bits >> v2) & 1u) << 2 | ((bits >> 7) & 1u) << 3;
}

__global__ __launch_bounds__(256) void mesh_count_kernel(const float* __restrict__ field, MeshDims d, float iso,
                                                         uint8_t* __restrict__ vflags, int* __restrict__ vcount,
                                                         int* __restrict__ tcount) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d.nx * d.ny * d.nz) return;
  const int iz = c % d.nz, iy = (c / d.nz) % d.ny, ix = c / (d.nz * d.ny);
  float val[8];
  const uint32_t bits = mesh_corners(field, d, c, ix, iy, iz, iso, val);
  const uint32_t f = mesh_vflags(bits);
  int nt = 0;
  if ((bits >> 8) == 0xFFu) {                 // all 8 corners exist: the cube does
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      const int n = __popc(mesh_tet_mask(bits, t));
      nt += n == 2 ? 2 : (n == 1 || n == 3) ? 1 : 0;
    }
  }
  vflags[c] = (uint8_t)f;
  vcount[c] = __popc(f);
  tcount[c] = nt;
}

__global__ __launch_bounds__(256) void mesh_emit_kernel(const float* __restrict__ field, MeshDims d, float iso,
                                                        float lo_x, float lo_y, float lo_z, float s_x, float s_y,
                                                        float s_z, const uint8_t* __restrict__ vflags,
                                                        const int* __restrict__ voff, const int* __restrict__ toff,
                                                        float* __restrict__ vert, int* __restrict__ tri) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d.nx * d.ny * d.nz) return;
  const int iz = c % d.nz, iy = (c / d.nz) % d.ny, ix = c / (d.nz * d.ny);
  float val[8];
  const uint32_t bits = mesh_corners(field, d, c, ix, iy, iz, iso, val);
  const uint32_t f = vflags[c];
  if (f) {
    // p_a = lo_a + float(i_a) s_a at this point (0) and one step up each axis (1)
    const float lo[3] = {lo_x, lo_y, lo_z}, s[3] = {s_x, s_y, s_z};
    const int i[3] = {ix, iy, iz};
    float p0[3], p1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      p0[a] = fadd_rn(lo[a], fmul_rn((float)i[a], s[a]));
      p1[a] = fadd_rn(lo[a], fmul_rn((float)(i[a] + 1), s[a]));
    }
    int row = voff[c];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      if (!((f >> k) & 1u)) continue;
      const int m = k + 1;
      float t = __fdiv_rn(fadd_rn(iso, -val[0]), fadd_rn(val[m], -val[0]));
      t = t != t ? 0.5f : t < 0.f ? 0.f : t > 1.f ? 1.f : t;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float pb = ((m >> (2 - a)) & 1) ? p1[a] : p0[a];
        vert[3 * (size_t)row + a] = fadd_rn(p0[a], fmul_rn(t, fadd_rn(pb, -p0[a])));
      }
      ++row;
    }
  }
  if ((bits >> 8) != 0xFFu) return;           // no cube at this point
  const uint32_t in = bits & 0xFFu;
  if (in == 0u || in == 0xFFu) return;        // no crossing in the cube
  // vertex row of edge k of the corner at offset code o
  int cvoff[8];
  uint32_t cvfl[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    const int co = c + (((o >> 2) & 1) * d.ny + ((o >> 1) & 1)) * d.nz + (o & 1);
    cvoff[o] = voff[co];
    cvfl[o] = vflags[co];
  }
  size_t out = 3 * (size_t)toff[c];
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const uint64_t e = kMeshTet[t * 16 + mesh_tet_mask(bits, t)];
    const int n = (int)(e & 3u);
    for (int j = 0; j < 3 * n; ++j) {
      const uint32_t ck = (uint32_t)(e >> (2 + 6 * j)) & 63u;
      const uint32_t o = ck >> 3, k = ck & 7u;
      int vo = cvoff[0];
      uint32_t vf = cvfl[0];
#pragma unroll
      for (int q = 1; q < 8; ++q)
        if (o == (uint32_t)q) {
          vo = cvoff[q];
          vf = cvfl[q];
        }
      tri[out++] = vo + __popc(vf & ((1u << k) - 1u));
    }
  }
}

}  // namespace cn
