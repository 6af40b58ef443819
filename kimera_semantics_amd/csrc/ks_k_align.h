// ks_k_align.h — scan-to-map pose refinement: a Gauss-Newton alignment of a point cloud (camera frame) to the zero level set
// of the device-resident TSDF.  The contract (the per-point f32 arithmetic, the 29 f64 sums and their order of summation, the
// LDL^T solve, the pose update, the state block) is DESIGN.md, section "Scan alignment"; tests/align_model.py restates it in
// NumPy and the kernels are compared with it bit for bit.
//
//   k_align_eval     one lane per USED point (point u * point_stride), 64 consecutive used points per wavefront.  A lane
//                    transforms its point by the pose in the state block, reads the first 8 bytes (distance, weight) of the
//                    eight corner records around it (one table lookup per tile through the renderer's per-lane memo), forms
//                    residual and Jacobian row in f32, their products in f64, and the wavefront folds the 30 values through six
//                    xor-shuffle steps.  Lane 0 stores the wavefront's partial at [sum][wavefront]: every partial of the
//                    launch is written, nothing is zeroed beforehand, no atomics.  The map is only read.
//   k_align_finish   ONE workgroup of 256: work-item j adds the partials j, j + 256, ... in ascending order, an LDS halving
//                    fold 128 .. 1 makes the totals, work-item 0 solves the 6 x 6 system (everything it indexes lies in LDS:
//                    no scratch) and updates pose, status and stats in the state block.
// An iteration is the pair (eval, finish); the host enqueues max_iterations pairs and one last pair that only fills the
// "last" stats.  The pairs of iterations after `done` was set return at once; the host reads nothing in between.
#pragma once
#include "ks_k_render.h"

namespace ksk {

constexpr int kAlignSums = 30;   // 21 J_a J_b (upper triangle, row-major) | 6 J_a r | r r | inliers | used points
constexpr double kAlignPivotRel = 0x1p-40;   // a pivot at or below this share of its diagonal entry is rounding noise: DEGENERATE
constexpr int kAlignLast = -1;   // the `iteration` argument of the pair that fills the "last" stats

struct AlignState {              // the device state block; the host writes it before the first pair and reads it after the last
  float q[4], t[3];              // the current pose T_G_C = (w, x, y, z), t
  uint32_t done, status, iterations;
  double used, inliers_first, rr_first, inliers_last, rr_last;   // (counts are integer-valued doubles)
};

struct AlignParams {
  const float* xyz;              // n points, camera frame
  uint32_t n, stride, n_used, n_waves;   // n_used = ceil(n / stride) lanes, n_waves = ceil(n_used / 64) partials
  float voxel_size_inv, min_weight, max_residual;
  uint32_t n_tiles;              // resident tiles: a slot at or above is no tile of the map
  float damping, eps_rotation, eps_translation;
  int32_t max_iterations, min_inliers;
  uint32_t dof_mask;
  double* partials;              // [kAlignSums][n_waves]
  AlignState* state;
};

// the eight corners of S(p) (as render_sample: the same g, corners and validity) kept for the gradient; a NaN distance is invalid
__device__ __forceinline__ bool align_corners(const TileTable& T, const Pool& P, const AlignParams& A, TileMemo& M, f3 p, float (&d)[8], float& fx,
                                              float& fy, float& fz) {
  const float gx = p.x * A.voxel_size_inv - 0.5f, gy = p.y * A.voxel_size_inv - 0.5f, gz = p.z * A.voxel_size_inv - 0.5f;
  const float ix = floorf(gx), iy = floorf(gy), iz = floorf(gz);
  const float lim = (float)(kCoordBias - 1);
  if (!(fabsf(ix) < lim && fabsf(iy) < lim && fabsf(iz) < lim && fabsf(ix + 1.0f) < lim && fabsf(iy + 1.0f) < lim && fabsf(iz + 1.0f) < lim))
    return false;
  fx = gx - ix;
  fy = gy - iy;
  fz = gz - iz;
  const int vx = (int)ix, vy = (int)iy, vz = (int)iz;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int x = vx + (k & 1), y = vy + ((k >> 1) & 1), z = vz + (k >> 2);
    const uint32_t slot = render_slot(T, M, x >> 3, y >> 3, z >> 3);
    uint2 q = make_uint2(0u, 0u);
    if (slot < A.n_tiles) {
      const uint32_t local = (uint32_t)(x & 7) + 8u * ((uint32_t)(y & 7) + 8u * (uint32_t)(z & 7));
      q = *(const uint2*)(P.vox + ((size_t)slot * kTileVoxels + local) * 8);
    } else {
      ok = false;
    }
    d[k] = __uint_as_float(q.x);
    ok = ok && __uint_as_float(q.y) >= A.min_weight && d[k] == d[k];
  }
  return ok;
}

// a + f * (b - a)
__device__ __forceinline__ float align_lerp(float a, float b, float f) { return a + f * (b - a); }

// grid ceil(n_used / 256) (at least 1), 256 work-items
__global__ void __launch_bounds__(256) k_align_eval(TileTable T, Pool P, AlignParams A, int iteration) {
  if (iteration != kAlignLast && A.state->done) return;
  const uint32_t lane = lane_id();
  const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (wave >= A.n_waves) return;   // (whole wavefronts: the last workgroup's spare ones)
  const uint32_t u = wave * 64u + lane;
  float J[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float r = 0.0f;
  double inlier = 0.0, used = 0.0;
  if (u < A.n_used) {
    const size_t i = (size_t)u * (size_t)A.stride;
    const f3 pc = {A.xyz[3 * i], A.xyz[3 * i + 1], A.xyz[3 * i + 2]};
    const float inf = __uint_as_float(0x7f800000u);
    if (fabsf(pc.x) < inf && fabsf(pc.y) < inf && fabsf(pc.z) < inf) {
      used = 1.0;
      Pose X;
      X.w = A.state->q[0];
      X.v = {A.state->q[1], A.state->q[2], A.state->q[3]};
      X.t = {A.state->t[0], A.state->t[1], A.state->t[2]};
      const f3 p = transform_point(X, pc);
      const f3 a = sub3(p, X.t);
      TileMemo M;
      float d[8], fx = 0.0f, fy = 0.0f, fz = 0.0f;
      if (align_corners(T, P, A, M, p, d, fx, fy, fz)) {
        const float s = align_lerp(align_lerp(align_lerp(d[0], d[1], fx), align_lerp(d[2], d[3], fx), fy),
                                   align_lerp(align_lerp(d[4], d[5], fx), align_lerp(d[6], d[7], fx), fy), fz);
        f3 g;
        g.x = align_lerp(align_lerp(d[1] - d[0], d[3] - d[2], fy), align_lerp(d[5] - d[4], d[7] - d[6], fy), fz) * A.voxel_size_inv;
        g.y = align_lerp(align_lerp(d[2] - d[0], d[3] - d[1], fx), align_lerp(d[6] - d[4], d[7] - d[5], fx), fz) * A.voxel_size_inv;
        g.z = align_lerp(align_lerp(d[4] - d[0], d[5] - d[1], fx), align_lerp(d[6] - d[2], d[7] - d[3], fx), fy) * A.voxel_size_inv;
        const float g2 = (g.x * g.x + g.y * g.y) + g.z * g.z;
        if (fabsf(s) < A.max_residual && g2 > 0.0f) {
          const f3 c = cross3(a, g);
          J[0] = c.x;
          J[1] = c.y;
          J[2] = c.z;
          J[3] = g.x;
          J[4] = g.y;
          J[5] = g.z;
          r = s;
          inlier = 1.0;
        }
      }
    }
  }
  // the wavefront is converged again.  A lane that is no inlier holds J = 0, r = 0: every product is +0.0
  double S[kAlignSums];
  {
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) S[k++] = (double)J[a] * (double)J[b];
#pragma unroll
    for (int a = 0; a < 6; ++a) S[21 + a] = (double)J[a] * (double)r;
    S[27] = (double)r * (double)r;
    S[28] = inlier;
    S[29] = used;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int k = 0; k < kAlignSums; ++k) S[k] += __shfl_xor(S[k], off);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kAlignSums; ++k) A.partials[(size_t)k * A.n_waves + wave] = S[k];
  }
}

// one workgroup of 256
__global__ void __launch_bounds__(256) k_align_finish(AlignParams A, int iteration) {
  __shared__ double sh[kAlignSums][256];
  __shared__ double H[6][6], L[6][6], D[6], b[6], y[6], x[6];
  AlignState* const st = A.state;
  if (iteration != kAlignLast && st->done) return;   // (uniform: the whole workgroup)
  const uint32_t j = threadIdx.x;
  {
    double acc[kAlignSums];
#pragma unroll
    for (int k = 0; k < kAlignSums; ++k) acc[k] = 0.0;
    for (uint32_t w = j; w < A.n_waves; w += 256u) {
#pragma unroll
      for (int k = 0; k < kAlignSums; ++k) acc[k] += A.partials[(size_t)k * A.n_waves + w];
    }
#pragma unroll
    for (int k = 0; k < kAlignSums; ++k) sh[k][j] = acc[k];
  }
  for (uint32_t off = 128; off >= 1; off >>= 1) {
    __syncthreads();
    for (uint32_t e = j; e < (uint32_t)kAlignSums * off; e += 256u) {
      const uint32_t k = e / off, i = e % off;
      sh[k][i] += sh[k][i + off];
    }
  }
  __syncthreads();
  if (j != 0) return;
  const double count = sh[28][0], rr = sh[27][0];
  if (iteration == kAlignLast) {
    st->inliers_last = count;
    st->rr_last = rr;
    return;
  }
  if (iteration == 0) {
    st->used = sh[29][0];
    st->inliers_first = count;
    st->rr_first = rr;
  }
  if (count < (double)A.min_inliers) {
    st->status = KS_ALIGN_TOO_FEW_INLIERS;
    st->done = 1u;
    return;
  }
  // mirror H, mask the degrees of freedom, damp
  {
    int k = 0;
    for (int a = 0; a < 6; ++a)
      for (int c = a; c < 6; ++c) {
        H[a][c] = sh[k][0];
        H[c][a] = sh[k][0];
        ++k;
      }
    for (int a = 0; a < 6; ++a) b[a] = sh[21 + a][0];
    for (int a = 0; a < 6; ++a)
      if (!((A.dof_mask >> a) & 1u)) {
        for (int c = 0; c < 6; ++c) {
          H[a][c] = 0.0;
          H[c][a] = 0.0;
        }
        H[a][a] = 1.0;
        b[a] = 0.0;
      }
    const double lambda = (double)A.damping * count;
    for (int a = 0; a < 6; ++a) H[a][a] = H[a][a] + lambda;
  }
  // H = L D L^T, column by column; a pivot that is not above 2^-40 of its diagonal entry (0, negative and NaN included) ends the loop
  for (int c = 0; c < 6; ++c) {
    double dj = H[c][c];
    for (int k = 0; k < c; ++k) dj = dj - (L[c][k] * D[k]) * L[c][k];
    if (!(dj > kAlignPivotRel * H[c][c])) {
      st->status = KS_ALIGN_DEGENERATE;
      st->done = 1u;
      return;
    }
    D[c] = dj;
    for (int i = c + 1; i < 6; ++i) {
      double v = H[i][c];
      for (int k = 0; k < c; ++k) v = v - (L[i][k] * D[k]) * L[c][k];
      L[i][c] = v / dj;
    }
  }
  for (int i = 0; i < 6; ++i) {   // L y = b, then y / D
    double v = b[i];
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v;
  }
  for (int i = 0; i < 6; ++i) y[i] = y[i] / D[i];
  for (int i = 5; i >= 0; --i) {   // L^T x = y
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
    x[i] = v;
  }
  const double d0 = -x[0], d1 = -x[1], d2 = -x[2], d3 = -x[3], d4 = -x[4], d5 = -x[5];
  // the pose update: dq = (1, omega / 2) from the left, renormalised; t + v
  const float hx = (float)d0 / 2.0f, hy = (float)d1 / 2.0f, hz = (float)d2 / 2.0f;
  const float qw = st->q[0], qx = st->q[1], qy = st->q[2], qz = st->q[3];
  const float nw = ((qw - hx * qx) - hy * qy) - hz * qz;
  const float nx = ((qx + hx * qw) + hy * qz) - hz * qy;
  const float ny = ((qy - hx * qz) + hy * qw) + hz * qx;
  const float nz = ((qz + hx * qy) - hy * qx) + hz * qw;
  const float len = sqrtf(((nw * nw + nx * nx) + ny * ny) + nz * nz);
  st->q[0] = nw / len;
  st->q[1] = nx / len;
  st->q[2] = ny / len;
  st->q[3] = nz / len;
  st->t[0] = st->t[0] + (float)d3;
  st->t[1] = st->t[1] + (float)d4;
  st->t[2] = st->t[2] + (float)d5;
  st->iterations = (uint32_t)iteration + 1u;
  const double er = (double)A.eps_rotation, et = (double)A.eps_translation;
  if ((d0 * d0 + d1 * d1) + d2 * d2 <= er * er && (d3 * d3 + d4 * d4) + d5 * d5 <= et * et) {
    st->status = KS_ALIGN_CONVERGED;
    st->done = 1u;
  } else if (iteration + 1 == A.max_iterations) {
    st->status = KS_ALIGN_ITERATION_LIMIT;
    st->done = 1u;
  }
}

}  // namespace ksk
