// ks_k_view_gain.h — view information gain over the stored ESDF: for each of n candidate camera poses, the DISTINCT voxels of
// each state (unknown, free, surface) that the fixed-step samples of a small pinhole image visit before a surface stops them.
// The contract (voxel states, rays, samples, the walk, the record, the box and the sizing rule) is DESIGN.md, section "View
// information gain"; tests/view_gain_model.py restates it in NumPy and the kernels are compared with it byte for byte.
// The ESDF store is only read.
//
//   k_vg_planes   pass 1, the only one that reads the 8-byte records: as k_fr_planes, a wavefront per z-layer of a tile (lane =
//                 x + 8 * y) and one ballot per fact.  A layer becomes four 64-bit words (32 B): observed | occupied | occupied
//                 and nearest_label == label | 0, so that a sample costs one tile lookup and one 16-byte load; the third word
//                 is read at a first visit of an occupied voxel only.
//   k_vg_walk     one workgroup per view in flight, persistent over the views with the grid as its stride.  Per view:
//                 1. every lane takes rays (an 8 x 8 pixel tile per wavefront, as k_render_view) and reduces the voxels of
//                    samples 0 and N - 1 to the view's voxel box: per axis p_k is monotone in k, so the two bound the ray;
//                 2. a visited bitmap over that box, one bit per voxel, in LDS when the box has at most lds_bits bits, else in
//                    the workgroup's slab of global memory (sized at the ball bound); only the box's words are zeroed;
//                 3. the walk: the lane whose atomic OR finds the bit clear counts the voxel, once, by its state; a read of the
//                    word skips the atomic where the bit is set already (on the global path an agent-scope load: a stale 0
//                    only falls through to the atomic, which decides);
//                 4. the seven counters: per wavefront by shuffles, then integer adds in LDS; lane 0 stores the record.
// Integer atomics only.  Which path a view takes changes the time and views_in_lds, never a record.
#pragma once
#include "ks_k_esdf_read.h"

namespace ksk {

constexpr uint32_t kVgThreads = 512;
constexpr uint32_t kVgLdsBits = 1u << 19;     // the LDS bitmap: 64 KiB of the CU's 160 KiB, two workgroups per CU
constexpr uint32_t kVgMaxGroups = 512;        // workgroups in flight: two per CU of a 256-CU device
constexpr uint32_t kVgLayerWords = 4;         // 64-bit words per z-layer of a tile
constexpr uint32_t kVgTileWords = 8 * kVgLayerWords;

struct VgParams {
  float cx, cy, constant_x, constant_y;
  int width, height;
  float voxel_size_inv, min_range, step, stop_distance;
  uint32_t n_samples;              // N
  uint32_t label;                  // 255: none
  uint32_t n_tiles;                // tiles of the ESDF store
  uint32_t n_views;
  uint32_t lds_bits;               // a box of at most this many bits takes the LDS path (<= kVgLdsBits)
  uint32_t pad;
  unsigned long long ball_bits;    // (2 * ceil(max_range / voxel_size) + 3)^3: what a slab holds, and a valid view's bound
  unsigned long long slab_words;   // uint32 words from one workgroup's slab to the next
};

struct VgCounters {   // 96 B
  unsigned long long views_valid, views_invalid, unknown, free_, surface, label, hit, open, samples, views_in_lds, pad[2];
};

static_assert(sizeof(ks_view_gain_record) == 32 && sizeof(ks_view_gain_config) == 56 && sizeof(ks_view_gain_stats) == 88, "ABI");
static_assert(sizeof(VgCounters) == 96, "layout");

// ---- pass 1: the bit planes ----------------------------------------------------------------------------------------------
// grid (nt * 2), 256 work-items: a wavefront is the z-layer (id >> 6) & 7 of tile id >> 9
__global__ void __launch_bounds__(256) k_vg_planes(const EsdfRecord* __restrict__ store, float stop_distance, uint32_t label,
                                                   unsigned long long* __restrict__ planes) {
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  const EsdfRecord r = store[id];
  const bool observed = (r.tail & 1u) != 0u;
  const bool occupied = observed && !(r.distance > stop_distance);   // (a NaN distance is occupied)
  const bool labelled = occupied && label != 255u && ((r.tail >> 8) & 0xffu) == label;
  const unsigned long long mo = __ballot(observed), mc = __ballot(occupied), ml = __ballot(labelled);
  const uint32_t lane = lane_id();
  if (lane < kVgLayerWords) planes[(size_t)(id >> 6) * kVgLayerWords + lane] = lane == 0 ? mo : lane == 1 ? mc : lane == 2 ? ml : 0ull;
}

// ---- the rays and their samples ----------------------------------------------------------------------------------------------
// ray slot r of a view: wavefront-sized groups of 8 x 8 pixels, row-major over the image.  False: no pixel (an edge tile).
// dg by the rule of k_render_view, operation for operation.
__device__ __forceinline__ bool vg_ray(const VgParams& V, const Pose& T, uint32_t r, f3& dg) {
  const uint32_t tiles_x = ((uint32_t)V.width + 7u) >> 3, tile = r >> 6, in = r & 63u;
  const int u = (int)((tile % tiles_x) * 8u + (in & 7u)), v = (int)((tile / tiles_x) * 8u + (in >> 3));
  if (u >= V.width || v >= V.height) return false;
  const float dcx = ((float)u - V.cx) * V.constant_x, dcy = ((float)v - V.cy) * V.constant_y;
  const float len = sqrtf((dcx * dcx + dcy * dcy) + 1.0f);
  const f3 uc = {dcx / len, dcy / len, 1.0f / len};
  dg = rotate_vector(T, uc);
  return true;
}

// p_k and its grid coordinates (floats, floored); false when a coordinate of p_k is not finite (the coordinates then bound only)
__device__ __forceinline__ bool vg_sample(const VgParams& V, const f3& o, const f3& dg, uint32_t k, float& cx, float& cy, float& cz) {
  const float t = V.min_range + (float)k * V.step;
  const float px = o.x + t * dg.x, py = o.y + t * dg.y, pz = o.z + t * dg.z;
  const float inf = __uint_as_float(0x7f800000u);
  cx = grid_coord(px, V.voxel_size_inv);
  cy = grid_coord(py, V.voxel_size_inv);
  cz = grid_coord(pz, V.voxel_size_inv);
  return fabsf(px) < inf && fabsf(py) < inf && fabsf(pz) < inf;
}
__device__ __forceinline__ bool vg_in_range(float cx, float cy, float cz) {
  const float lim = (float)(kCoordBias - 1);
  return fabsf(cx) < lim && fabsf(cy) < lim && fabsf(cz) < lim;
}
// a coordinate of sample N - 1 as a bound: beyond the packed range (or infinite) it is the last index a sample can have
__device__ __forceinline__ int vg_clamped(float c) {
  const float last = (float)(kCoordBias - 2);
  return (int)fminf(fmaxf(c, -last), last);
}

__device__ __forceinline__ int vg_wave_min(int v) {
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int vg_wave_max(int v) {
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

struct VgBox {
  int x0, y0, z0;
  uint32_t nx, ny, nz;
};

// the walk of one view over a bitmap in LDS (LDS = true) or in the workgroup's slab; c[7]: unknown | free | surface | label |
// hit | open | samples of this lane's rays
template <bool LDS>
__device__ __forceinline__ void vg_walk_view(const TileTable& T, const VgParams& V, const Pose& P, const VgBox& B,
                                             const unsigned long long* __restrict__ planes, uint32_t* bits, uint32_t n_slots, uint32_t c[7]) {
  for (uint32_t r = threadIdx.x; r < n_slots; r += kVgThreads) {
    f3 dg;
    if (!vg_ray(V, P, r, dg)) continue;
    TileMemo M;
    bool hit = false;
    for (uint32_t k = 0; k < V.n_samples; ++k) {
      float fx, fy, fz;
      if (!vg_sample(V, P.t, dg, k, fx, fy, fz) || !vg_in_range(fx, fy, fz)) break;
      const int x = (int)fx, y = (int)fy, z = (int)fz;
      const uint32_t lx = (uint32_t)(x - B.x0), ly = (uint32_t)(y - B.y0), lz = (uint32_t)(z - B.z0);
      if (lx >= B.nx || ly >= B.ny || lz >= B.nz) break;   // (never: samples 0 and N - 1 bound the ray; no word outside the bitmap is touched)
      ++c[6];
      const uint32_t slot = render_slot(T, M, x >> 3, y >> 3, z >> 3);
      const unsigned long long* layer = planes;
      ulonglong2 q = make_ulonglong2(0ull, 0ull);   // (no tile of the store: the default record, unknown)
      if (slot < V.n_tiles) {
        layer = planes + ((size_t)slot * 8u + (uint32_t)(z & 7)) * kVgLayerWords;
        q = *(const ulonglong2*)layer;
      }
      const uint32_t b = (uint32_t)(x & 7) + 8u * (uint32_t)(y & 7);
      const bool observed = ((q.x >> b) & 1ull) != 0ull, occupied = ((q.y >> b) & 1ull) != 0ull;
      const size_t at = ((size_t)lz * B.ny + ly) * B.nx + lx;
      uint32_t* word = bits + (at >> 5);
      const uint32_t m = 1u << (uint32_t)(at & 31u);
      const uint32_t seen = LDS ? *(volatile uint32_t*)word : __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!(seen & m) && !(atomicOr(word, m) & m)) {   // this lane set the bit: it counts the voxel
        if (!observed) ++c[0];
        else if (!occupied) ++c[1];
        else {
          ++c[2];
          if (V.label != 255u && ((layer[2] >> b) & 1ull)) ++c[3];
        }
      }
      if (occupied) {
        hit = true;
        break;
      }
    }
    c[4] += hit ? 1u : 0u;
    c[5] += hit ? 0u : 1u;
  }
}

// grid (groups), kVgThreads work-items
__global__ void __launch_bounds__(kVgThreads) k_vg_walk(TileTable T, VgParams V, const float* __restrict__ poses,
                                                        const unsigned long long* __restrict__ planes, uint32_t* __restrict__ slabs,
                                                        ks_view_gain_record* __restrict__ out, VgCounters* __restrict__ C) {
  __shared__ uint32_t s_bits[kVgLdsBits / 32];
  __shared__ int s_lo[3], s_hi[3];
  __shared__ uint32_t s_cnt[7];
  const uint32_t tid = threadIdx.x, lane = lane_id();
  const uint32_t n_slots = (((uint32_t)V.width + 7u) >> 3) * (((uint32_t)V.height + 7u) >> 3) * 64u;
  uint32_t* slab = slabs + (size_t)blockIdx.x * V.slab_words;
  if (tid < 7u) s_cnt[tid] = 0u;
  for (uint32_t view = blockIdx.x; view < V.n_views; view += gridDim.x) {
    const float* p = poses + (size_t)view * 7u;
    Pose P;
    P.w = p[0];
    P.v = {p[1], p[2], p[3]};
    P.t = {p[4], p[5], p[6]};
    const float inf = __uint_as_float(0x7f800000u);
    bool valid = true;   // (uniform)
    for (int k = 0; k < 7; ++k) valid = valid && fabsf(p[k]) < inf;
    if (tid < 3u) s_lo[tid] = 0x7fffffff, s_hi[tid] = (int)0x80000000;
    __syncthreads();
    // 1) the box
    if (valid) {
      int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
      for (uint32_t r = tid; r < n_slots; r += kVgThreads) {
        f3 dg;
        float a[3], b[3];
        if (!vg_ray(V, P, r, dg) || !vg_sample(V, P.t, dg, 0u, a[0], a[1], a[2]) || !vg_in_range(a[0], a[1], a[2])) continue;   // a ray without a sample
        // (p_0 is finite, so dg is: a coordinate of p_(N-1) that is not finite is an overflow, an infinity on dg's side of p_0)
        (void)vg_sample(V, P.t, dg, V.n_samples - 1u, b[0], b[1], b[2]);
        for (int k = 0; k < 3; ++k) {
          const int v0 = (int)a[k], v1 = vg_clamped(b[k]);
          lo[k] = min(lo[k], min(v0, v1));
          hi[k] = max(hi[k], max(v0, v1));
        }
      }
      for (int k = 0; k < 3; ++k) {
        const int l = vg_wave_min(lo[k]), h = vg_wave_max(hi[k]);
        if (lane == 0 && l <= h) {
          atomicMin(&s_lo[k], l);
          atomicMax(&s_hi[k], h);
        }
      }
    }
    __syncthreads();
    // 2) the bitmap
    VgBox B{s_lo[0], s_lo[1], s_lo[2], 0u, 0u, 0u};
    unsigned long long n_bits = 0;
    if (valid && s_lo[0] <= s_hi[0]) {
      B.nx = (uint32_t)(s_hi[0] - s_lo[0]) + 1u, B.ny = (uint32_t)(s_hi[1] - s_lo[1]) + 1u, B.nz = (uint32_t)(s_hi[2] - s_lo[2]) + 1u;
      n_bits = (unsigned long long)B.nx * B.ny * B.nz;
    }
    if (n_bits > V.ball_bits) valid = false;   // rays that leave the ball of max_range: no unit quaternion
    const bool in_lds = n_bits <= (unsigned long long)V.lds_bits;
    if (valid && n_bits) {
      const size_t n_words = (size_t)((n_bits + 31ull) >> 5);
      if (in_lds) {
        for (size_t w = tid; w < n_words; w += kVgThreads) s_bits[w] = 0u;
      } else {
        for (size_t w = tid; w < n_words; w += kVgThreads) slab[w] = 0u;
        __threadfence();   // the zeroes are in L2 before another lane's atomic OR
      }
    }
    __syncthreads();
    // 3) the walk, 4) its sums
    uint32_t c[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (valid) {
      if (in_lds) vg_walk_view<true>(T, V, P, B, planes, s_bits, n_slots, c);
      else vg_walk_view<false>(T, V, P, B, planes, slab, n_slots, c);
    }
    for (int k = 0; k < 7; ++k) {
      uint32_t s = c[k];
      for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
      if (lane == 0 && s) atomicAdd(&s_cnt[k], s);
    }
    __syncthreads();
    if (tid == 0) {
      ks_view_gain_record R{};
      if (valid) {
        R.unknown_voxels = s_cnt[0], R.free_voxels = s_cnt[1], R.surface_voxels = s_cnt[2], R.label_voxels = s_cnt[3];
        R.rays_hit = s_cnt[4], R.rays_open = s_cnt[5], R.samples = s_cnt[6];
        R.flags = KS_VIEW_GAIN_VALID;
        atomicAdd(&C->views_valid, 1ull);
        atomicAdd(&C->unknown, (unsigned long long)s_cnt[0]);
        atomicAdd(&C->free_, (unsigned long long)s_cnt[1]);
        atomicAdd(&C->surface, (unsigned long long)s_cnt[2]);
        atomicAdd(&C->label, (unsigned long long)s_cnt[3]);
        atomicAdd(&C->hit, (unsigned long long)s_cnt[4]);
        atomicAdd(&C->open, (unsigned long long)s_cnt[5]);
        atomicAdd(&C->samples, (unsigned long long)s_cnt[6]);
        if (in_lds && n_bits) atomicAdd(&C->views_in_lds, 1ull);
      } else {
        atomicAdd(&C->views_invalid, 1ull);
      }
      out[view] = R;
      for (int k = 0; k < 7; ++k) s_cnt[k] = 0u;   // (the next view's adds come after three more barriers)
    }
  }
}

}  // namespace ksk
