// ks_k_esdf.h — ESDF with nearest-surface labels from the device-resident map: the batch update and the incremental
// refresh.  The contract (observed voxels, sites, the integer window, the 64-bit key, the final f32 rule) is DESIGN.md,
// section "ESDF"; tests/esdf_model.py restates it in NumPy and the kernels are compared with it bit for bit.
//
// The key of a site is  d2 << 40 | bits(|distance|) << 8 | label  and the result of a voxel is the MINIMUM key over the
// same-sign sites of its (2R+1)^3 window.  d2 = dx^2 + dy^2 + dz^2 and adding dx^2 << 40 keeps the order of the rest, so
// the 3-D minimum is three 1-D windowed minima in a row, each a brute-force minimum over 2R+1 keys from LDS:
//
//   k_esdf_fill      default records into the store of every resident tile
//   k_esdf_x         reads (distance, weight, label) of the 128-byte records through the dense slot grid of the box; one
//                    wavefront per row, 64 voxels along x, the row segment with a halo of R staged in LDS for both signs;
//                    writes two keys per voxel (plane 0: sites with distance >= 0, plane 1: distance < 0)
//   k_esdf_axis<0>   pass y, box to box: 16 voxels along x (one 128-byte line of keys) times 64 along y per workgroup, the
//                    window staged in chunks of 64 rows
//   k_esdf_axis<1>   pass z: the same walk along z over the plane of the voxel's own sign, then the final rule and the
//                    8-byte record into the store of the voxel's tile (resident tiles, inside the region, only)
//   k_esdf_download  host-layout blocks of records;  k_esdf_query  nearest-voxel lookup of world points
//   k_esdf_brick<0|1|2>  the same three passes over lists of tile positions, for the incremental refresh (further down);
//   k_esdf_count     the totals of a store from its records
//
// A plane never holds all-ones for "no site": kEsdfNone = 1 << 62 is above every real key (d2 <= 3 * 255^2 < 2^18) and
// stays below 2^63 after the three additions, so the passes need no special case.
#pragma once
#include "ks_types.h"

namespace ksk {

constexpr uint64_t kEsdfNone = 1ull << 62;
constexpr int kEsdfMaxR = 255;
constexpr int kEsdfRowLen = 64 + 2 * kEsdfMaxR + 2;   // 576 keys: one row segment of pass x with its halo
constexpr int kEsdfChunk = 64;                        // rows of the window staged at a time by passes y and z
constexpr int kEsdfPer = 4;                           // outputs along the axis per work-item of passes y and z

struct EsdfBox {
  int nx, ny, nz;           // voxels of the box (multiples of 8); coordinates below count from its first voxel
  int r0[3], r1[3];         // voxels [r0, r1) that get results (the region; the whole box without one)
  int R;
  float voxel_size, min_weight, min_distance, max_distance;
  const uint32_t* slots;    // [nz/8][ny/8][nx/8] pool slot of the tile, 0xffffffff where none is resident
};

struct EsdfRecord {
  float distance;
  uint32_t tail;            // flags | nearest_label << 8 (two bytes of padding above)
};
constexpr uint32_t kEsdfDefaultTail = 255u << 8;

__global__ void __launch_bounds__(256) k_esdf_fill(EsdfRecord* __restrict__ store, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) store[i] = EsdfRecord{0.0f, kEsdfDefaultTail};
}

__device__ __forceinline__ uint32_t esdf_slot(const EsdfBox& B, int x, int y, int z) {
  return B.slots[((size_t)(z >> 3) * (size_t)(B.ny >> 3) + (size_t)(y >> 3)) * (size_t)(B.nx >> 3) + (size_t)(x >> 3)];
}
__device__ __forceinline__ uint32_t esdf_local(int x, int y, int z) {
  return (uint32_t)(x & 7) + 8u * ((uint32_t)(y & 7) + 8u * (uint32_t)(z & 7));
}

// grid (ceil(nx / 64), ceil(ny / 4), nz), 256 work-items: wavefront w takes the row (y0 + w, z)
__global__ void __launch_bounds__(256) k_esdf_x(EsdfBox B, Pool P, uint64_t* __restrict__ out) {
  __shared__ uint64_t s_key[2][4][kEsdfRowLen];
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  const int x0 = (int)blockIdx.x * 64, y = (int)blockIdx.y * 4 + (int)wave, z = (int)blockIdx.z;
  const int R = B.R, len = 64 + 2 * R;
  if (y < B.ny) {
    for (int i = (int)lane; i < len; i += 64) {
      const int x = x0 - R + i;
      uint64_t kpos = kEsdfNone, kneg = kEsdfNone;
      if (x >= 0 && x < B.nx) {
        const uint32_t slot = esdf_slot(B, x, y, z);
        if (slot != 0xffffffffu) {
          const uint4 q = P.vox[((size_t)slot * kTileVoxels + esdf_local(x, y, z)) * 8];
          const float d = __uint_as_float(q.x), w = __uint_as_float(q.y);
          if (w >= B.min_weight && fabsf(d) < B.min_distance) {
            const uint32_t label = q.w == 255u ? 0u : (q.w & 0xffu);
            const uint64_t k = ((uint64_t)__float_as_uint(fabsf(d)) << 8) | (uint64_t)label;
            if (d < 0.0f) kneg = k;
            else kpos = k;
          }
        }
      }
      s_key[0][wave][i] = kpos;
      s_key[1][wave][i] = kneg;
    }
  }
  __syncthreads();
  const int x = x0 + (int)lane;
  if (y >= B.ny || x >= B.nx) return;
  uint64_t m0 = kEsdfNone, m1 = kEsdfNone;
  const uint64_t* r0 = &s_key[0][wave][R + (int)lane];
  const uint64_t* r1 = &s_key[1][wave][R + (int)lane];
  for (int o = -R; o <= R; ++o) {
    const uint64_t add = (uint64_t)(uint32_t)(o * o) << 40;
    const uint64_t a = r0[o] + add, b = r1[o] + add;
    m0 = a < m0 ? a : m0;
    m1 = b < m1 ? b : m1;
  }
  const size_t nvox = (size_t)B.nx * (size_t)B.ny * (size_t)B.nz;
  const size_t at = ((size_t)z * (size_t)B.ny + (size_t)y) * (size_t)B.nx + (size_t)x;
  out[at] = m0;
  out[nvox + at] = m1;
}

// Passes y (FINAL = 0) and z (FINAL = 1).  256 work-items = 16 along x times 16 along the axis, kEsdfPer outputs each: a
// workgroup owns 16 x 64 voxels of one plane perpendicular to the third axis.  grid (nx / 16, ceil(n_axis / 64), n_other).
// counters (FINAL): voxels observed | fixed | clamped.
template <int FINAL>
__global__ void __launch_bounds__(256) k_esdf_axis(EsdfBox B, Pool P, const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                   EsdfRecord* __restrict__ store, unsigned long long* __restrict__ counters) {
  __shared__ uint64_t s_key[2][kEsdfChunk][16];
  const int lx = (int)(threadIdx.x & 15u), la = (int)(threadIdx.x >> 4);
  const int x = (int)blockIdx.x * 16 + lx;            // (nx is a multiple of 8: a workgroup may hang over by 8)
  const int other = (int)blockIdx.z;                  // z in pass y, y in pass z
  const int n_axis = FINAL ? B.nz : B.ny;
  const int a0 = (int)blockIdx.y * (16 * kEsdfPer);
  const size_t nvox = (size_t)B.nx * (size_t)B.ny * (size_t)B.nz;
  const size_t stride = FINAL ? (size_t)B.nx * (size_t)B.ny : (size_t)B.nx;
  const size_t base = FINAL ? (size_t)other * (size_t)B.nx : (size_t)other * (size_t)B.nx * (size_t)B.ny;
  const int R = B.R;
  const bool in_x = x < B.nx;
  // the outputs of this work-item: a = a0 + la + 16 * j; in pass z the voxel's own record decides the plane it reads
  int plane[kEsdfPer];
  float dist[kEsdfPer];
  uint32_t slot[kEsdfPer];
  bool observed[kEsdfPer], site[kEsdfPer], live[kEsdfPer];
  uint32_t own_label[kEsdfPer];
  uint64_t m0[kEsdfPer], m1[kEsdfPer];
#pragma unroll
  for (int j = 0; j < kEsdfPer; ++j) {
    const int a = a0 + la + 16 * j;
    m0[j] = m1[j] = kEsdfNone;
    plane[j] = 0;
    dist[j] = 0.0f;
    slot[j] = 0xffffffffu;
    observed[j] = site[j] = false;
    own_label[j] = 0u;
    live[j] = in_x && a < n_axis;
    if (FINAL && live[j]) {
      const int y = other, z = a;
      const bool in_region = x >= B.r0[0] && x < B.r1[0] && y >= B.r0[1] && y < B.r1[1] && z >= B.r0[2] && z < B.r1[2];
      slot[j] = in_region ? esdf_slot(B, x, y, z) : 0xffffffffu;
      live[j] = slot[j] != 0xffffffffu;
      if (live[j]) {
        const uint4 q = P.vox[((size_t)slot[j] * kTileVoxels + esdf_local(x, y, z)) * 8];
        const float d = __uint_as_float(q.x), w = __uint_as_float(q.y);
        dist[j] = d;
        observed[j] = w >= B.min_weight;
        site[j] = observed[j] && fabsf(d) < B.min_distance;
        plane[j] = d < 0.0f ? 1 : 0;
        own_label[j] = q.w == 255u ? 0u : (q.w & 0xffu);
      }
    }
  }
  // the window of the workgroup's 64 outputs, in chunks of kEsdfChunk rows
  const int w_lo = max(a0 - R, 0), w_hi = min(a0 + 16 * kEsdfPer - 1 + R, n_axis - 1);
  for (int c0 = w_lo; c0 <= w_hi; c0 += kEsdfChunk) {
    __syncthreads();
    for (int i = (int)threadIdx.x; i < kEsdfChunk * 16; i += 256) {
      const int row = i >> 4, cx = (int)blockIdx.x * 16 + (i & 15), a = c0 + row;
      uint64_t k0 = kEsdfNone, k1 = kEsdfNone;
      if (a <= w_hi && cx < B.nx) {
        const size_t at = base + (size_t)a * stride + (size_t)cx;
        k0 = in[at];
        k1 = in[nvox + at];
      }
      s_key[0][row][i & 15] = k0;
      s_key[1][row][i & 15] = k1;
    }
    __syncthreads();
    const int c1 = min(c0 + kEsdfChunk - 1, w_hi);
#pragma unroll
    for (int j = 0; j < kEsdfPer; ++j) {
      const int a = a0 + la + 16 * j;
      const int lo = max(a - R, c0), hi = min(a + R, c1);
      if (FINAL) {
        const uint64_t* col = &s_key[plane[j]][0][lx];
        uint64_t m = m0[j];
        for (int r = lo; r <= hi; ++r) {
          const int o = r - a;
          const uint64_t k = col[(r - c0) * 16] + ((uint64_t)(uint32_t)(o * o) << 40);
          m = k < m ? k : m;
        }
        m0[j] = m;
      } else {
        uint64_t ma = m0[j], mb = m1[j];
        for (int r = lo; r <= hi; ++r) {
          const int o = r - a;
          const uint64_t add = (uint64_t)(uint32_t)(o * o) << 40;
          const uint64_t ka = s_key[0][r - c0][lx] + add, kb = s_key[1][r - c0][lx] + add;
          ma = ka < ma ? ka : ma;
          mb = kb < mb ? kb : mb;
        }
        m0[j] = ma;
        m1[j] = mb;
      }
    }
  }
  uint32_t n_obs = 0, n_fix = 0, n_clamp = 0;
#pragma unroll
  for (int j = 0; j < kEsdfPer; ++j) {
    const int a = a0 + la + 16 * j;
    if (!FINAL) {
      if (live[j]) {
        const size_t at = base + (size_t)a * stride + (size_t)x;
        out[at] = m0[j];
        out[nvox + at] = m1[j];
      }
    } else {
      bool clamped = false;
      if (live[j]) {
        EsdfRecord rec{0.0f, kEsdfDefaultTail};
        if (site[j]) {
          rec.distance = dist[j];
          rec.tail = 3u | (own_label[j] << 8);
        } else if (observed[j]) {
          const uint64_t k = m0[j];
          float d = B.max_distance;
          uint32_t label = 255u;
          clamped = true;
          if (k < kEsdfNone) {
            const float centre = B.voxel_size * sqrtf((float)(uint32_t)(k >> 40));
            const float sum = centre + __uint_as_float((uint32_t)(k >> 8));
            clamped = !(sum < B.max_distance);
            d = fminf(B.max_distance, sum);
            label = (uint32_t)(k & 0xffu);
          }
          rec.distance = plane[j] ? -d : d;
          rec.tail = 1u | (label << 8);
        }
        store[(size_t)slot[j] * kTileVoxels + esdf_local(x, other, a)] = rec;
      }
      n_obs += (uint32_t)__popcll(__ballot(live[j] && observed[j]));
      n_fix += (uint32_t)__popcll(__ballot(live[j] && site[j]));
      n_clamp += (uint32_t)__popcll(__ballot(clamped));
    }
  }
  if (FINAL && lane_id() == 0) {
    if (n_obs) atomicAdd(&counters[0], (unsigned long long)n_obs);
    if (n_fix) atomicAdd(&counters[1], (unsigned long long)n_fix);
    if (n_clamp) atomicAdd(&counters[2], (unsigned long long)n_clamp);
  }
}

// Host-layout export: one lane per voxel of a host block (the layout of k_download).  n_tiles = tiles resident at the update:
// a tile that joined the map later reads as default records.
__global__ void __launch_bounds__(256) k_esdf_download(TileTable T, const EsdfRecord* __restrict__ store, uint32_t n_tiles,
                                                       const int32_t* __restrict__ block_idx, int vps, EsdfRecord* __restrict__ out) {
  const uint32_t b = blockIdx.y;
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nv = (uint32_t)(vps * vps * vps);
  if (l >= nv) return;
  const int lx = (int)(l % (uint32_t)vps), ly = (int)((l / (uint32_t)vps) % (uint32_t)vps), lz = (int)(l / (uint32_t)(vps * vps));
  const int vx = block_idx[3 * b] * vps + lx, vy = block_idx[3 * b + 1] * vps + ly, vz = block_idx[3 * b + 2] * vps + lz;
  EsdfRecord rec{0.0f, kEsdfDefaultTail};
  const int tx = vx >> 3, ty = vy >> 3, tz = vz >> 3;
  if (tx >= -kTileBias && tx < kTileBias && ty >= -kTileBias && ty < kTileBias && tz >= -kTileBias && tz < kTileBias) {
    const uint32_t slot = tile_lookup(T, pack_tile(tx, ty, tz));
    if (slot < n_tiles) rec = store[(size_t)slot * kTileVoxels + esdf_local(vx, vy, vz)];
  }
  out[(size_t)b * nv + l] = rec;
}

// Nearest-voxel lookup: the voxel of a point is the one the integrator takes for a ray's end point (grid_coord).
__global__ void __launch_bounds__(256) k_esdf_query(TileTable T, const EsdfRecord* __restrict__ store, uint32_t n_tiles,
                                                    const float* __restrict__ xyz, size_t n, float voxel_size_inv,
                                                    EsdfRecord* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float gx = grid_coord(xyz[3 * i], voxel_size_inv), gy = grid_coord(xyz[3 * i + 1], voxel_size_inv),
              gz = grid_coord(xyz[3 * i + 2], voxel_size_inv);
  EsdfRecord rec{0.0f, kEsdfDefaultTail};
  const float lim = (float)(kCoordBias - 1);
  if (fabsf(gx) < lim && fabsf(gy) < lim && fabsf(gz) < lim) {
    const int vx = (int)gx, vy = (int)gy, vz = (int)gz;
    const uint32_t slot = tile_lookup(T, pack_tile(vx >> 3, vy >> 3, vz >> 3));
    if (slot < n_tiles) rec = store[(size_t)slot * kTileVoxels + esdf_local(vx, vy, vz)];
  }
  out[i] = rec;
}

// ---- incremental refresh (ks_esdf_refresh; DESIGN.md, "ESDF", incremental refresh) -----------------------------------------
// The same three passes over LISTS of tile positions instead of a box.  A listed position owns a BRICK: the two key planes of
// its 8^3 voxels, [sign][z][y][x], 8 KiB.  Pass x (AXIS 0) makes the bricks of list X from the records of the resident tiles
// beside each position along x (found through the context's tile table), pass y the bricks of list Y from those of X, pass z
// the final records of the tiles of list Z from those of Y; a brick is found by bisection in the sorted positions of the list
// it belongs to, and a miss reads as "no sites".  One workgroup per position.  The window along the axis is walked one
// neighbour brick at a time through LDS, so LDS does not depend on R: s_key[sign][index along the axis][the other two].  The
// passes read it with lanes on consecutive 8-byte words.  Staging a brick writes it transposed; an 8-byte LDS write goes 16
// lanes at a time over 32 banks, and the rows are padded so that those 16 lanes fall on 16 different words: pass x stages
// 8 indices along the axis times 2 rows across (row stride = 2 words mod 16: 66), pass y 2 along times 8 across (8 mod 16: 72).
// A list position is pack_coord3 of a tile's coordinates: they are dilated by up to 2 * 32 tiles, beyond the 18-bit fields of a tile key.
constexpr int kEsdfBrickKeys = 2 * kTileVoxels;

struct EsdfRefresh {
  int R;
  float voxel_size, min_weight, min_distance, max_distance;
};

__device__ __forceinline__ uint32_t esdf_find(const uint64_t* __restrict__ keys, uint32_t n, uint64_t k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && keys[lo] == k ? lo : 0xffffffffu;
}

// element e of a brick (x + 8 * (y + 8 * z)) -> its index along AXIS and over the other two coordinates, and back
template <int AXIS>
__device__ __forceinline__ void esdf_split(uint32_t e, uint32_t& along, uint32_t& across) {
  if (AXIS == 0) { along = e & 7u; across = e >> 3; }
  else if (AXIS == 1) { along = (e >> 3) & 7u; across = (e & 7u) | ((e >> 6) << 3); }
  else { along = e >> 6; across = e & 63u; }
}

// grid (positions of the list), 256 work-items: lane = the voxel's index across the axis, wavefront w = outputs 2w and 2w + 1
// along it.  pos: the list (sorted); AXIS 0: n_tiles = resident tiles, in / in_pos unused; AXIS 1, 2: in = the bricks of the
// list in_pos[n_in]; AXIS 0, 1: out = this list's bricks; AXIS 2: slots = pool slot of each position, store = the records.
template <int AXIS>
__global__ void __launch_bounds__(256) k_esdf_brick(EsdfRefresh E, TileTable T, Pool P, uint32_t n_tiles, const uint64_t* __restrict__ pos,
                                                    const uint64_t* __restrict__ in_pos, uint32_t n_in, const uint64_t* __restrict__ in,
                                                    uint64_t* __restrict__ out, const uint32_t* __restrict__ slots,
                                                    EsdfRecord* __restrict__ store) {
  constexpr int kRow = AXIS == 0 ? 66 : 72;
  __shared__ uint64_t s_key[2][8][kRow];
  const uint32_t b = blockIdx.x, across = lane_id(), wave = threadIdx.x >> 6;
  int tx, ty, tz;
  unpack_coord3(pos[b], tx, ty, tz);
  const int R = E.R, g = (R + 7) >> 3;
  // pass z: the voxel's own record decides the plane it reads
  uint32_t slot = 0;
  int plane[2] = {0, 0};
  float dist[2] = {0.0f, 0.0f};
  bool observed[2] = {false, false}, site[2] = {false, false};
  uint32_t own_label[2] = {0u, 0u};
  if (AXIS == 2) {
    slot = slots[b];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint4 q = P.vox[((size_t)slot * kTileVoxels + across + 64u * (2u * wave + (uint32_t)j)) * 8];
      const float d = __uint_as_float(q.x), w = __uint_as_float(q.y);
      dist[j] = d;
      observed[j] = w >= E.min_weight;
      site[j] = observed[j] && fabsf(d) < E.min_distance;
      plane[j] = d < 0.0f ? 1 : 0;
      own_label[j] = q.w == 255u ? 0u : (q.w & 0xffu);
    }
  }
  uint64_t m0[2] = {kEsdfNone, kEsdfNone}, m1[2] = {kEsdfNone, kEsdfNone};
  for (int dt = -g; dt <= g; ++dt) {   // (every neighbour within g tiles has an offset within R: 8 * g - 7 <= R)
    // the neighbour's keys: the same for every work-item, so the branches below do not diverge
    const int nx = tx + (AXIS == 0 ? dt : 0), ny = ty + (AXIS == 1 ? dt : 0), nz = tz + (AXIS == 2 ? dt : 0);
    uint32_t src;
    if (AXIS == 0) {
      src = 0xffffffffu;
      if (nx >= -kTileBias && nx < kTileBias && ny >= -kTileBias && ny < kTileBias && nz >= -kTileBias && nz < kTileBias)
        src = tile_lookup(T, pack_tile(nx, ny, nz));
      if (src >= n_tiles) continue;
    } else {
      src = esdf_find(in_pos, n_in, pack_coord3(nx, ny, nz));
      if (src == 0xffffffffu) continue;
    }
    __syncthreads();   // (the brick staged before this one has been read)
    for (uint32_t e = threadIdx.x; e < (uint32_t)kTileVoxels; e += 256u) {
      uint64_t k0 = kEsdfNone, k1 = kEsdfNone;
      if (AXIS == 0) {
        const uint4 q = P.vox[((size_t)src * kTileVoxels + e) * 8];
        const float d = __uint_as_float(q.x), w = __uint_as_float(q.y);
        if (w >= E.min_weight && fabsf(d) < E.min_distance) {
          const uint32_t label = q.w == 255u ? 0u : (q.w & 0xffu);
          const uint64_t k = ((uint64_t)__float_as_uint(fabsf(d)) << 8) | (uint64_t)label;
          if (d < 0.0f) k1 = k;
          else k0 = k;
        }
      } else {
        k0 = in[(size_t)src * kEsdfBrickKeys + e];
        k1 = in[(size_t)src * kEsdfBrickKeys + kTileVoxels + e];
      }
      uint32_t i, c;
      esdf_split<AXIS>(e, i, c);
      s_key[0][i][c] = k0;
      s_key[1][i][c] = k1;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int a = 2 * (int)wave + j;
      uint64_t ma = m0[j], mb = m1[j];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int o = dt * 8 + i - a;
        if (o < -R || o > R) continue;
        const uint64_t add = (uint64_t)(uint32_t)(o * o) << 40;
        if (AXIS == 2) {
          const uint64_t k = s_key[plane[j]][i][across] + add;
          ma = k < ma ? k : ma;
        } else {
          const uint64_t ka = s_key[0][i][across] + add, kb = s_key[1][i][across] + add;
          ma = ka < ma ? ka : ma;
          mb = kb < mb ? kb : mb;
        }
      }
      m0[j] = ma;
      m1[j] = mb;
    }
  }
  if (AXIS != 2) {
    // through LDS once more, so that the brick leaves in its own order: consecutive work-items, consecutive words
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      s_key[0][2 * wave + j][across] = m0[j];
      s_key[1][2 * wave + j][across] = m1[j];
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < (uint32_t)kTileVoxels; e += 256u) {
      uint32_t i, c;
      esdf_split<AXIS>(e, i, c);
      out[(size_t)b * kEsdfBrickKeys + e] = s_key[0][i][c];
      out[(size_t)b * kEsdfBrickKeys + kTileVoxels + e] = s_key[1][i][c];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      EsdfRecord rec{0.0f, kEsdfDefaultTail};
      if (site[j]) {
        rec.distance = dist[j];
        rec.tail = 3u | (own_label[j] << 8);
      } else if (observed[j]) {
        const uint64_t k = m0[j];
        float d = E.max_distance;
        uint32_t label = 255u;
        if (k < kEsdfNone) {
          const float centre = E.voxel_size * sqrtf((float)(uint32_t)(k >> 40));
          const float sum = centre + __uint_as_float((uint32_t)(k >> 8));
          d = fminf(E.max_distance, sum);
          label = (uint32_t)(k & 0xffu);
        }
        rec.distance = plane[j] ? -d : d;
        rec.tail = 1u | (label << 8);
      }
      store[(size_t)slot * kTileVoxels + across + 64u * (2u * wave + (uint32_t)j)] = rec;
    }
  }
}

// voxels observed | fixed | clamped of a store, from its records (the totals ks_esdf_update counts while it writes them):
// 1024 records per workgroup
__global__ void __launch_bounds__(256) k_esdf_count(const EsdfRecord* __restrict__ store, size_t n, float max_distance,
                                                    unsigned long long* __restrict__ counters) {
  uint32_t n_obs = 0, n_fix = 0, n_clamp = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const size_t i = (size_t)blockIdx.x * 1024u + (size_t)j * 256u + threadIdx.x;
    bool obs = false, fix = false, clamped = false;
    if (i < n) {
      const EsdfRecord r = store[i];
      obs = (r.tail & 1u) != 0u;
      fix = (r.tail & 2u) != 0u;
      clamped = obs && !fix && fabsf(r.distance) == max_distance;
    }
    n_obs += (uint32_t)__popcll(__ballot(obs));
    n_fix += (uint32_t)__popcll(__ballot(fix));
    n_clamp += (uint32_t)__popcll(__ballot(clamped));
  }
  if (lane_id() == 0) {
    if (n_obs) atomicAdd(&counters[0], (unsigned long long)n_obs);
    if (n_fix) atomicAdd(&counters[1], (unsigned long long)n_fix);
    if (n_clamp) atomicAdd(&counters[2], (unsigned long long)n_clamp);
  }
}

}  // namespace ksk
