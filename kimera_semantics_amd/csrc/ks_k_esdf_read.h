// ks_k_esdf_read.h — what a planner reads of the stored ESDF, where the records are: trilinear distance and gradient at
// arbitrary points, slice images, and segments swept against a robot radius.  The contract (the sample E(p), the slice's pixel
// positions, the sweep's walk, outputs and statistics; the order of every f32 operation) is DESIGN.md, section "ESDF reads";
// tests/esdf_read_model.py restates it in NumPy and the kernels are compared with it bit for bit.  The store is only read, as it
// is: (TileTable, store, n_tiles) address it exactly as k_esdf_query does, nothing is refreshed.
//
//   k_esdf_sample   one lane per point.  E(p) reads the 8-byte records of the eight corner voxels and of the point's own voxel;
//                   a lane remembers the tile it looked up last (TileMemo, ks_k_render.h), so the nine records of a sample
//                   inside one tile cost one table lookup.
//   k_esdf_slice    one lane per pixel of a plane origin + i du + j dv; a wavefront covers 8 x 8 pixels and a workgroup 2 x 2 of
//                   them, as k_render_view, so neighbouring lanes read the same 64-byte rows of the store.
//   k_esdf_sweep    one lane per segment: sphere-steps along it by the clearance E(p) - radius, at least min_step, in a for loop
//                   of at most max_samples iterations.  Lengths diverge inside a wavefront; the lane's TileMemo carries from one
//                   sample to the next.
// No LDS, no floating-point atomics: the counters are integer sums, one atomic per wavefront per counter.
#pragma once
#include "ks_k_align.h"
#include "ks_k_esdf.h"
#include "ks_k_render.h"

namespace ksk {

struct EsdfReadStore {
  const EsdfRecord* records;   // [n_tiles][512]
  uint32_t n_tiles;            // tiles that were resident when the store was made: a slot at or above reads as a default record
  float voxel_size_inv;
};

struct EsdfSampleOut {         // any may be nullptr
  float* distance;             // [n]
  float* gradient;             // [n][3]
  uint8_t* status;             // [n]  0 unknown | 1 nearest | 2 interpolated
  uint8_t* label;              // [n]
  uint8_t* flags;              // [n]
  unsigned long long* counters;   // interpolated | nearest | unknown
};

struct EsdfSlice {
  float origin[3], du[3], dv[3];
  int width, row0, rows;       // this launch takes the rows [row0, row0 + rows); the outputs start at row row0
};

struct EsdfSweep {
  const float* segments;       // [n][6]  a, b
  size_t n;
  float radius, min_step, max_length;   // max_length = (float)(max_samples - 2) * min_step
  int32_t unknown_is_free, max_samples;
  uint8_t* status;             // [n]   any of the four may be nullptr
  float* t_stop;               // [n]
  float* min_clearance;        // [n]
  float* t_min;                // [n]
  unsigned long long* counters;   // free | collision | unknown | invalid | samples
};

struct EsdfSampleValue {
  uint32_t status;             // 0 | 1 | 2
  float distance;
  f3 gradient;
  uint32_t tail;               // flags | label << 8 of the point's own voxel (the default tail when the status is 0)
};

// the record of voxel (x, y, z), every coordinate inside the packed range
__device__ __forceinline__ uint2 esdf_read_record(const TileTable& T, const EsdfReadStore& S, TileMemo& M, int x, int y, int z) {
  const uint32_t slot = render_slot(T, M, x >> 3, y >> 3, z >> 3);
  uint2 q = make_uint2(0u, kEsdfDefaultTail);
  if (slot < S.n_tiles) q = *(const uint2*)(S.records + ((size_t)slot * kTileVoxels + esdf_local(x, y, z)));
  return q;
}

// E(p).  GRAD = false leaves the gradient at (0, 0, 0) whatever the status (the sweep needs the distance only).
template <bool GRAD>
__device__ __forceinline__ EsdfSampleValue esdf_read_sample(const TileTable& T, const EsdfReadStore& S, TileMemo& M, float px, float py, float pz) {
  EsdfSampleValue E;
  E.status = 0u;
  E.distance = __uint_as_float(0x7fc00000u);
  E.gradient = {0.0f, 0.0f, 0.0f};
  E.tail = kEsdfDefaultTail;
  const float inf = __uint_as_float(0x7f800000u);
  if (!(fabsf(px) < inf && fabsf(py) < inf && fabsf(pz) < inf)) return E;
  const float gx = px * S.voxel_size_inv - 0.5f, gy = py * S.voxel_size_inv - 0.5f, gz = pz * S.voxel_size_inv - 0.5f;
  const float ix = floorf(gx), iy = floorf(gy), iz = floorf(gz);
  const float lim = (float)(kCoordBias - 1);
  if (!(fabsf(ix) < lim && fabsf(iy) < lim && fabsf(iz) < lim && fabsf(ix + 1.0f) < lim && fabsf(iy + 1.0f) < lim && fabsf(iz + 1.0f) < lim))
    return E;
  const float fx = gx - ix, fy = gy - iy, fz = gz - iz;
  const int vx = (int)ix, vy = (int)iy, vz = (int)iz;
  float d[8];
  bool all = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint2 q = esdf_read_record(T, S, M, vx + (k & 1), vy + ((k >> 1) & 1), vz + (k >> 2));
    d[k] = __uint_as_float(q.x);
    all = all && (q.y & 1u);
  }
  // the point's own voxel, as k_esdf_query takes it
  const float nx = grid_coord(px, S.voxel_size_inv), ny = grid_coord(py, S.voxel_size_inv), nz = grid_coord(pz, S.voxel_size_inv);
  uint2 own = make_uint2(0u, kEsdfDefaultTail);
  if (fabsf(nx) < lim && fabsf(ny) < lim && fabsf(nz) < lim) own = esdf_read_record(T, S, M, (int)nx, (int)ny, (int)nz);
  if (all) {
    E.status = 2u;
    E.distance = align_lerp(align_lerp(align_lerp(d[0], d[1], fx), align_lerp(d[2], d[3], fx), fy),
                            align_lerp(align_lerp(d[4], d[5], fx), align_lerp(d[6], d[7], fx), fy), fz);
    if (GRAD) {
      E.gradient.x = align_lerp(align_lerp(d[1] - d[0], d[3] - d[2], fy), align_lerp(d[5] - d[4], d[7] - d[6], fy), fz) * S.voxel_size_inv;
      E.gradient.y = align_lerp(align_lerp(d[2] - d[0], d[3] - d[1], fx), align_lerp(d[6] - d[4], d[7] - d[5], fx), fz) * S.voxel_size_inv;
      E.gradient.z = align_lerp(align_lerp(d[4] - d[0], d[5] - d[1], fx), align_lerp(d[6] - d[2], d[7] - d[3], fx), fy) * S.voxel_size_inv;
    }
    E.tail = own.y;
  } else if (own.y & 1u) {
    E.status = 1u;
    E.distance = __uint_as_float(own.x);
    E.tail = own.y;
  }
  return E;
}

__device__ __forceinline__ void esdf_read_store(const EsdfSampleOut& O, size_t at, const EsdfSampleValue& E) {
  if (O.distance) O.distance[at] = E.distance;
  if (O.gradient) {
    O.gradient[3 * at] = E.gradient.x;
    O.gradient[3 * at + 1] = E.gradient.y;
    O.gradient[3 * at + 2] = E.gradient.z;
  }
  if (O.status) O.status[at] = (uint8_t)E.status;
  if (O.label) O.label[at] = (uint8_t)((E.tail >> 8) & 0xffu);
  if (O.flags) O.flags[at] = (uint8_t)(E.tail & 0xffu);
}

// the wavefront is converged: its three sums, one atomic each
__device__ __forceinline__ void esdf_read_count(unsigned long long* counters, bool live, uint32_t status) {
  const unsigned long long m2 = __ballot(live && status == 2u), m1 = __ballot(live && status == 1u), m0 = __ballot(live && status == 0u);
  if (lane_id() == 0) {
    if (m2) atomicAdd(&counters[0], (unsigned long long)__popcll(m2));
    if (m1) atomicAdd(&counters[1], (unsigned long long)__popcll(m1));
    if (m0) atomicAdd(&counters[2], (unsigned long long)__popcll(m0));
  }
}

// grid ceil(n / 256), 256 work-items
__global__ void __launch_bounds__(256) k_esdf_sample(TileTable T, EsdfReadStore S, const float* __restrict__ xyz, size_t n, EsdfSampleOut O) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  const bool live = i < n;
  uint32_t status = 0u;
  if (live) {
    TileMemo M;
    const EsdfSampleValue E = esdf_read_sample<true>(T, S, M, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    esdf_read_store(O, i, E);
    status = E.status;
  }
  esdf_read_count(O.counters, live, status);
}

// grid (ceil(width / 16), ceil(rows / 16)), 256 work-items: wavefront w takes the 8 x 8 pixels at (w & 1, w >> 1) of the 16 x 16
__global__ void __launch_bounds__(256) k_esdf_slice(TileTable T, EsdfReadStore S, EsdfSlice V, EsdfSampleOut O) {
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  const int i = (int)blockIdx.x * 16 + (int)(wave & 1u) * 8 + (int)(lane & 7u);
  const int r = (int)blockIdx.y * 16 + (int)(wave >> 1) * 8 + (int)(lane >> 3);
  const bool live = i < V.width && r < V.rows;
  uint32_t status = 0u;
  if (live) {
    const float fi = (float)i, fj = (float)(V.row0 + r);
    const float px = (V.origin[0] + fi * V.du[0]) + fj * V.dv[0];
    const float py = (V.origin[1] + fi * V.du[1]) + fj * V.dv[1];
    const float pz = (V.origin[2] + fi * V.du[2]) + fj * V.dv[2];
    TileMemo M;
    const EsdfSampleValue E = esdf_read_sample<true>(T, S, M, px, py, pz);
    esdf_read_store(O, (size_t)r * (size_t)V.width + (size_t)i, E);
    status = E.status;
  }
  esdf_read_count(O.counters, live, status);
}

// grid ceil(n / 256), 256 work-items.  THE WALK BELOW HAS A SECOND COPY: path_sweep of ks_k_path.h restates it operation for operation
// (without t_stop and t_min) for k_path_shorten, because factoring it out changed this kernel's instruction stream.  Both are compared
// bit for bit with the one sweep of tests/esdf_read_model.py; a change to the walk goes into both.
__global__ void __launch_bounds__(256) k_esdf_sweep(TileTable T, EsdfReadStore S, EsdfSweep W) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  const bool live = i < W.n;
  const float inf = __uint_as_float(0x7f800000u);
  uint32_t status = 3u;   // KS_SWEEP_INVALID
  int samples = 0;
  if (live) {
    const float ax = W.segments[6 * i], ay = W.segments[6 * i + 1], az = W.segments[6 * i + 2];
    const float bx = W.segments[6 * i + 3], by = W.segments[6 * i + 4], bz = W.segments[6 * i + 5];
    const float dx = bx - ax, dy = by - ay, dz = bz - az;
    const float L = sqrtf((dx * dx + dy * dy) + dz * dz);
    float t_stop = 0.0f, min_c = inf, t_min = 0.0f;
    const bool finite = fabsf(ax) < inf && fabsf(ay) < inf && fabsf(az) < inf && fabsf(bx) < inf && fabsf(by) < inf && fabsf(bz) < inf && L < inf;
    if (finite && !(L > W.max_length)) {
      const bool point = L == 0.0f;
      const float ux = point ? 0.0f : dx / L, uy = point ? 0.0f : dy / L, uz = point ? 0.0f : dz / L;
      TileMemo M;
      float t = 0.0f;
      // every step but the last is at least min_step and L <= (max_samples - 2) * min_step: the loop ends by one of its three exits
      // (a segment that rounding keeps from it stays INVALID)
      for (int it = 0; it < W.max_samples; ++it) {
        const EsdfSampleValue E = esdf_read_sample<false>(T, S, M, ax + t * ux, ay + t * uy, az + t * uz);
        ++samples;
        if (E.status == 0u && !W.unknown_is_free) {
          status = 2u;   // KS_SWEEP_UNKNOWN
          t_stop = t;
          break;
        }
        float c = 0.0f;
        if (E.status != 0u) {
          c = E.distance - W.radius;
          if (c < min_c) {
            min_c = c;
            t_min = t;
          }
          if (c < 0.0f) {
            status = 1u;   // KS_SWEEP_COLLISION
            t_stop = t;
            break;
          }
        }
        if (t >= L) {
          status = 0u;   // KS_SWEEP_FREE
          t_stop = L;
          break;
        }
        const float step = E.status != 0u ? fmaxf(c, W.min_step) : W.min_step;
        t = fminf(t + step, L);
      }
      if (status == 3u) {   // (the bound: the outputs of an INVALID segment)
        t_stop = 0.0f;
        min_c = inf;
        t_min = 0.0f;
      }
    }
    if (W.status) W.status[i] = (uint8_t)status;
    if (W.t_stop) W.t_stop[i] = t_stop;
    if (W.min_clearance) W.min_clearance[i] = min_c;
    if (W.t_min) W.t_min[i] = t_min;
  }
  // the wavefront is converged again: its five sums, one atomic each
  const unsigned long long m_free = __ballot(live && status == 0u), m_col = __ballot(live && status == 1u);
  const unsigned long long m_unk = __ballot(live && status == 2u), m_inv = __ballot(live && status == 3u);
  for (int off = 32; off >= 1; off >>= 1) samples += __shfl_xor(samples, off);
  if (lane_id() == 0) {
    if (m_free) atomicAdd(&W.counters[0], (unsigned long long)__popcll(m_free));
    if (m_col) atomicAdd(&W.counters[1], (unsigned long long)__popcll(m_col));
    if (m_unk) atomicAdd(&W.counters[2], (unsigned long long)__popcll(m_unk));
    if (m_inv) atomicAdd(&W.counters[3], (unsigned long long)__popcll(m_inv));
    if (samples) atomicAdd(&W.counters[4], (unsigned long long)samples);
  }
}

}  // namespace ksk
