// ks_k_render.h — depth, label, colour and normal images of the device-resident map from a camera pose: one ray per pixel,
// sphere-traced through the resident tiles with trilinear samples of the TSDF.  The contract (ray, sample, march, outputs,
// stats; the order of every f32 operation) is DESIGN.md, section "View rendering"; tests/render_model.py restates it in NumPy
// and the kernel is compared with it bit for bit.
//
//   k_render_view   one lane per pixel; a wavefront covers an 8 x 8 pixel tile and a workgroup 2 x 2 of them, so the samples
//                   of neighbouring lanes fall into the same or adjacent voxels — the same 128-byte records.  A sample reads
//                   the first 8 bytes (distance, weight) of its eight corner records; a lane remembers the tile it looked up
//                   last, so the eight corners of a sample inside one tile, and consecutive samples in it, cost one table
//                   lookup (the table is read-only here: the remembered slot is what a fresh lookup returns).  The map is
//                   only read.  No LDS; the three counters take one atomic per wavefront each (integer sums).
#pragma once
#include "ks_types.h"

namespace ksk {

struct RenderView {
  Pose T;                      // T_G_C
  float cx, cy, constant_x, constant_y;
  int width, height;
  float voxel_size, voxel_size_inv, min_weight, min_range, max_range;
  uint32_t n_tiles;            // resident tiles: a slot at or above is no tile of the map
  float* depth;                // [h][w]      any of the four may be nullptr
  uint8_t* labels;             // [h][w]
  uint32_t* rgba;              // [h][w]
  float* normals;              // [h][w][3]
  unsigned long long* counters;   // pixels hit | pixels missed | march samples
};

// the rotation of transform_point (ks_device_math.h), without the translation
__device__ __forceinline__ f3 rotate_vector(const Pose& T, f3 p) {
  f3 uv = cross3(T.v, p);
  uv = add3(uv, uv);
  const f3 c2 = cross3(T.v, uv);
  f3 r;
  r.x = (p.x + T.w * uv.x) + c2.x;
  r.y = (p.y + T.w * uv.y) + c2.y;
  r.z = (p.z + T.w * uv.z) + c2.z;
  return r;
}

struct TileMemo {   // the last tile a lane looked up
  uint64_t key = kEmpty64;   // (no tile packs to all-ones)
  uint32_t slot = 0xffffffffu;
};

__device__ __forceinline__ uint32_t render_slot(const TileTable& T, TileMemo& M, int tx, int ty, int tz) {
  const uint64_t key = pack_tile(tx, ty, tz);
  if (key != M.key) {
    M.key = key;
    M.slot = tile_lookup(T, key);
  }
  return M.slot;
}

// S(p): trilinear TSDF sample; false when a corner is outside the packed range, in no resident tile or below min_weight
__device__ __forceinline__ bool render_sample(const TileTable& T, const Pool& P, const RenderView& V, TileMemo& M, float px, float py,
                                              float pz, float& s) {
  const float gx = px * V.voxel_size_inv - 0.5f, gy = py * V.voxel_size_inv - 0.5f, gz = pz * V.voxel_size_inv - 0.5f;
  const float ix = floorf(gx), iy = floorf(gy), iz = floorf(gz);
  const float lim = (float)(kCoordBias - 1);
  if (!(fabsf(ix) < lim && fabsf(iy) < lim && fabsf(iz) < lim && fabsf(ix + 1.0f) < lim && fabsf(iy + 1.0f) < lim && fabsf(iz + 1.0f) < lim))
    return false;
  const float fx = gx - ix, fy = gy - iy, fz = gz - iz;
  const int vx = (int)ix, vy = (int)iy, vz = (int)iz;
  float d[8];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int x = vx + (k & 1), y = vy + ((k >> 1) & 1), z = vz + (k >> 2);
    const uint32_t slot = render_slot(T, M, x >> 3, y >> 3, z >> 3);
    uint2 q = make_uint2(0u, 0u);
    if (slot < V.n_tiles) {
      const uint32_t local = (uint32_t)(x & 7) + 8u * ((uint32_t)(y & 7) + 8u * (uint32_t)(z & 7));
      q = *(const uint2*)(P.vox + ((size_t)slot * kTileVoxels + local) * 8);
    } else {
      ok = false;
    }
    d[k] = __uint_as_float(q.x);
    ok = ok && __uint_as_float(q.y) >= V.min_weight;
  }
  if (!ok) return false;
  const float a0 = d[0] + fx * (d[1] - d[0]), a1 = d[2] + fx * (d[3] - d[2]);
  const float a2 = d[4] + fx * (d[5] - d[4]), a3 = d[6] + fx * (d[7] - d[6]);
  const float b0 = a0 + fy * (a1 - a0), b1 = a2 + fy * (a3 - a2);
  s = b0 + fz * (b1 - b0);
  return true;
}

// grid (ceil(width / 16), ceil(height / 16)), 256 work-items: wavefront w takes the 8 x 8 pixels at (w & 1, w >> 1) of the 16 x 16
__global__ void __launch_bounds__(256) k_render_view(TileTable T, Pool P, RenderView V) {
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  const int u = (int)blockIdx.x * 16 + (int)(wave & 1u) * 8 + (int)(lane & 7u);
  const int v = (int)blockIdx.y * 16 + (int)(wave >> 1) * 8 + (int)(lane >> 3);
  const bool live = u < V.width && v < V.height;   // (edge tiles: the other lanes march nothing and store nothing)
  bool hit = false;
  int samples = 0;
  if (live) {
    const float dcx = ((float)u - V.cx) * V.constant_x, dcy = ((float)v - V.cy) * V.constant_y;
    const float len = sqrtf((dcx * dcx + dcy * dcy) + 1.0f);
    const f3 uc = {dcx / len, dcy / len, 1.0f / len};
    const f3 dg = rotate_vector(V.T, uc);
    const f3 o = V.T.t;
    TileMemo M;
    float r = V.min_range, r_prev = 0.0f, s_prev = 0.0f, r_hit = 0.0f;
    bool prev_pos = false;
    // every step is at least one voxel and max_range / voxel_size <= 4096 (ks_render_view): at most 4097 samples
    while (!(r > V.max_range)) {
      ++samples;
      float s = 0.0f;
      const bool valid = render_sample(T, P, V, M, o.x + r * dg.x, o.y + r * dg.y, o.z + r * dg.z, s);
      if (valid && s <= 0.0f && prev_pos) {
        r_hit = r_prev + (r - r_prev) * (s_prev / (s_prev - s));
        hit = true;
        break;
      }
      prev_pos = valid && s > 0.0f;
      if (prev_pos) {
        r_prev = r;
        s_prev = s;
      }
      r += prev_pos ? fmaxf(s, V.voxel_size) : V.voxel_size;
    }
    float depth = __uint_as_float(0x7fc00000u);
    uint32_t label = 255u, rgba = 0u;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (hit) {
      const float hx = o.x + r_hit * dg.x, hy = o.y + r_hit * dg.y, hz = o.z + r_hit * dg.z;
      depth = r_hit * uc.z;
      label = 0u;
      if (V.labels || V.rgba) {
        const float cxf = grid_coord(hx, V.voxel_size_inv), cyf = grid_coord(hy, V.voxel_size_inv), czf = grid_coord(hz, V.voxel_size_inv);
        const float lim = (float)(kCoordBias - 1);
        if (fabsf(cxf) < lim && fabsf(cyf) < lim && fabsf(czf) < lim) {
          const int x = (int)cxf, y = (int)cyf, z = (int)czf;
          const uint32_t slot = render_slot(T, M, x >> 3, y >> 3, z >> 3);
          if (slot < V.n_tiles) {
            const uint32_t local = (uint32_t)(x & 7) + 8u * ((uint32_t)(y & 7) + 8u * (uint32_t)(z & 7));
            const uint4 q = P.vox[((size_t)slot * kTileVoxels + local) * 8];
            rgba = q.z;
            label = q.w == 255u ? 0u : (q.w & 0xffu);
          }
        }
      }
      if (V.normals) {
        const float h = V.voxel_size;
        float sp[3], sm[3];
        bool ok = render_sample(T, P, V, M, hx + h, hy, hz, sp[0]);
        ok = ok && render_sample(T, P, V, M, hx - h, hy, hz, sm[0]);
        ok = ok && render_sample(T, P, V, M, hx, hy + h, hz, sp[1]);
        ok = ok && render_sample(T, P, V, M, hx, hy - h, hz, sm[1]);
        ok = ok && render_sample(T, P, V, M, hx, hy, hz + h, sp[2]);
        ok = ok && render_sample(T, P, V, M, hx, hy, hz - h, sm[2]);
        if (ok) {
          const float gx = sp[0] - sm[0], gy = sp[1] - sm[1], gz = sp[2] - sm[2];
          const float n2 = (gx * gx + gy * gy) + gz * gz;
          if (n2 > 0.0f) {
            const float n = sqrtf(n2);
            nx = gx / n;
            ny = gy / n;
            nz = gz / n;
          }
        }
      }
    }
    const size_t at = (size_t)v * (size_t)V.width + (size_t)u;
    if (V.depth) V.depth[at] = depth;
    if (V.labels) V.labels[at] = (uint8_t)label;
    if (V.rgba) V.rgba[at] = rgba;
    if (V.normals) {
      V.normals[3 * at] = nx;
      V.normals[3 * at + 1] = ny;
      V.normals[3 * at + 2] = nz;
    }
  }
  // the wavefront is converged again: its three sums, one atomic each
  const unsigned long long m_hit = __ballot(live && hit), m_miss = __ballot(live && !hit);
  for (int off = 32; off >= 1; off >>= 1) samples += __shfl_xor(samples, off);
  if (lane == 0) {
    if (m_hit) atomicAdd(&V.counters[0], (unsigned long long)__popcll(m_hit));
    if (m_miss) atomicAdd(&V.counters[1], (unsigned long long)__popcll(m_miss));
    if (samples) atomicAdd(&V.counters[2], (unsigned long long)samples);
  }
}

}  // namespace ksk
