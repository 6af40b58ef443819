// ks_k_fuse.h — resampling one resident map under a rigid pose into the grid of another (ks_fuse_map).
//   k_fuse_resample   one workgroup per candidate DESTINATION tile, one lane per destination voxel: the voxel's centre goes through
//                     T_S_D into the source frame, the source TSDF is sampled there trilinearly (the renderer's S(p): the same g,
//                     corners and validity, plus "no NaN distance"), and the tile leaves as an exchange-format tile (ks_k_io.h:
//                     what k_merge_tiles takes; label 255 = untouched) in the work space, with the number of touched voxels.
//                     The up to 3 x 3 x 3 source tiles a destination tile reads are looked up ONCE per workgroup into LDS (a
//                     sample would otherwise cost up to eight table lookups); a sample reads the first 8 bytes of eight records,
//                     and only a valid voxel reads the whole 128-byte record of its nearest corner — in the 8-lanes-per-voxel,
//                     16-bytes-per-lane shape of the other tile kernels, so record reads and writes are whole 128-byte lines.
//                     A tile with no touched voxel writes its count and nothing else.
//   k_fuse_flag       one lane per touched tile: the two sync flags k_merge_tiles leaves to its callers.
// Both maps are only read by k_fuse_resample; the fold itself is k_merge_tiles, unchanged.
#pragma once
#include "ks_types.h"

namespace ksk {

struct FuseView {
  Pose T;                      // T_S_D: destination frame -> source frame
  float voxel_size, voxel_size_inv, min_weight;
  uint32_t n_src_tiles;        // resident tiles of the source: a slot at or above is no tile of it
};

constexpr uint32_t kFuseNone = 0xffffffffu;

__global__ void __launch_bounds__(512) k_fuse_resample(TileTable S, Pool SP, FuseView V, const uint64_t* __restrict__ cand,
                                                        uint4* __restrict__ out, uint32_t* __restrict__ counts) {
  __shared__ int s_lo[3];             // lowest source tile any in-range corner of this workgroup lies in
  __shared__ uint32_t s_slot[27];     // the source slots of the 3 x 3 x 3 tiles from s_lo on (kFuseNone: not resident)
  __shared__ uint32_t s_cnt;
  __shared__ float s_d[kTileVoxels], s_w[kTileVoxels];
  __shared__ uint32_t s_rec[kTileVoxels];   // source record (slot * 512 + local) of the nearest corner; kFuseNone: untouched
  const uint32_t tid = threadIdx.x;
  if (tid < 3) s_lo[tid] = 0x7fffffff;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  int tx, ty, tz;
  unpack_tile(cand[blockIdx.x], tx, ty, tz);
  // 2. the point: the centre of the destination voxel in the source frame
  const int vx = tx * 8 + (int)(tid & 7u), vy = ty * 8 + (int)((tid >> 3) & 7u), vz = tz * 8 + (int)(tid >> 6);
  const f3 c = {((float)vx + 0.5f) * V.voxel_size, ((float)vy + 0.5f) * V.voxel_size, ((float)vz + 0.5f) * V.voxel_size};
  const f3 p = transform_point(V.T, c);
  // 3. the sample
  const float gx = p.x * V.voxel_size_inv - 0.5f, gy = p.y * V.voxel_size_inv - 0.5f, gz = p.z * V.voxel_size_inv - 0.5f;
  const float ix = floorf(gx), iy = floorf(gy), iz = floorf(gz);
  const float lim = (float)(kCoordBias - 1);
  const bool in_range = fabsf(ix) < lim && fabsf(iy) < lim && fabsf(iz) < lim && fabsf(ix + 1.0f) < lim && fabsf(iy + 1.0f) < lim && fabsf(iz + 1.0f) < lim;
  const float fx = gx - ix, fy = gy - iy, fz = gz - iz;
  const int x0 = in_range ? (int)ix : 0, y0 = in_range ? (int)iy : 0, z0 = in_range ? (int)iz : 0;
  if (in_range) {
    atomicMin(&s_lo[0], x0 >> 3);
    atomicMin(&s_lo[1], y0 >> 3);
    atomicMin(&s_lo[2], z0 >> 3);
  }
  __syncthreads();
  const int lx = s_lo[0], ly = s_lo[1], lz = s_lo[2];
  if (tid < 27 && lx != 0x7fffffff) {
    const int sx = lx + (int)(tid % 3u), sy = ly + (int)((tid / 3u) % 3u), sz = lz + (int)(tid / 9u);
    uint32_t slot = kFuseNone;
    if (sx < kTileBias && sy < kTileBias && sz < kTileBias) {   // (not below -kTileBias: an in-range corner lies in it or above)
      slot = tile_lookup(S, pack_tile(sx, sy, sz));
      if (slot >= V.n_src_tiles) slot = kFuseNone;
    }
    s_slot[tid] = slot;
  }
  __syncthreads();
  bool ok = in_range;
  float d[8], w[8];
  uint32_t rec[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int x = x0 + (k & 1), y = y0 + ((k >> 1) & 1), z = z0 + (k >> 2);
    const int dx = (x >> 3) - lx, dy = (y >> 3) - ly, dz = (z >> 3) - lz;
    uint32_t slot = kFuseNone;
    if (in_range) {
      if (dx < 3 && dy < 3 && dz < 3) {   // (dx, dy, dz >= 0: s_lo is the minimum)
        slot = s_slot[dx + 3 * (dy + 3 * dz)];
      } else {   // a span of more than three tiles: not with a rigid pose, but no index may depend on that
        slot = tile_lookup(S, pack_tile(x >> 3, y >> 3, z >> 3));
        if (slot >= V.n_src_tiles) slot = kFuseNone;
      }
    }
    uint2 q = make_uint2(0u, 0u);
    rec[k] = kFuseNone;
    if (slot != kFuseNone) {
      rec[k] = slot * (uint32_t)kTileVoxels + ((uint32_t)(x & 7) + 8u * ((uint32_t)(y & 7) + 8u * (uint32_t)(z & 7)));
      q = *(const uint2*)(SP.vox + (size_t)rec[k] * 8);
    } else {
      ok = false;
    }
    d[k] = __uint_as_float(q.x);
    w[k] = __uint_as_float(q.y);
    ok = ok && w[k] >= V.min_weight && !(d[k] != d[k]);
  }
  const float a0 = d[0] + fx * (d[1] - d[0]), a1 = d[2] + fx * (d[3] - d[2]);
  const float a2 = d[4] + fx * (d[5] - d[4]), a3 = d[6] + fx * (d[7] - d[6]);
  const float b0 = a0 + fy * (a1 - a0), b1 = a2 + fy * (a3 - a2);
  const float da = b0 + fz * (b1 - b0);
  const float e0 = w[0] + fx * (w[1] - w[0]), e1 = w[2] + fx * (w[3] - w[2]);
  const float e2 = w[4] + fx * (w[5] - w[4]), e3 = w[6] + fx * (w[7] - w[6]);
  const float g0 = e0 + fy * (e1 - e0), g1 = e2 + fy * (e3 - e2);
  const float wa = g0 + fz * (g1 - g0);
  const int nk = (fx >= 0.5f ? 1 : 0) | (fy >= 0.5f ? 2 : 0) | (fz >= 0.5f ? 4 : 0);
  uint32_t nrec = rec[0];
#pragma unroll
  for (int k = 1; k < 8; ++k)
    if (nk == k) nrec = rec[k];
  s_d[tid] = da;
  s_w[tid] = wa;
  s_rec[tid] = ok ? nrec : kFuseNone;
  const unsigned long long m = __ballot(ok);
  if (lane_id() == 0 && m) atomicAdd(&s_cnt, (uint32_t)__popcll(m));
  __syncthreads();
  const uint32_t total = s_cnt;
  if (tid == 0) counts[blockIdx.x] = total;
  if (total == 0) return;   // (the whole workgroup: nothing of this tile is read by anyone)
  // 4. the incoming records: 8 lanes per voxel, 16 bytes per lane
  uint4* tile = out + (size_t)blockIdx.x * kTileVoxels * 8;
  const uint32_t sub = tid & 7u;
  const uint32_t pi = __float_as_uint(kPriorInit);
#pragma unroll
  for (uint32_t r = 0; r < 8; ++r) {
    const uint32_t q = r * 512u + tid, vox = q >> 3;
    const uint32_t from = s_rec[vox];
    uint4 v;
    if (from != kFuseNone) {
      v = SP.vox[(size_t)from * 8 + sub];
      if (sub == 0u) {
        v.x = __float_as_uint(s_d[vox]);
        v.y = __float_as_uint(s_w[vox]);
        if (v.w == 255u) v.w = 0u;
      } else if (sub == 6u) {
        v.y = v.z = v.w = 0u;
      } else if (sub == 7u) {
        v = make_uint4(0u, 0u, 0u, 0u);
      }
    } else {   // untouched: the empty record of k_reset_tiles
      if (sub == 0u) v = make_uint4(0u, 0u, 0u, 255u);
      else if (sub < 6u) v = make_uint4(pi, pi, pi, pi);
      else if (sub == 6u) v = make_uint4(pi, 0u, 0u, 0u);
      else v = make_uint4(0u, 0u, 0u, 0u);
    }
    tile[q] = v;
  }
}

// the tiles k_merge_tiles folded into: it marks them stale for the mesher and the ESDF and leaves the two sync flags to its caller
__global__ void __launch_bounds__(256) k_fuse_flag(TileTable T, Pool P, const uint64_t* __restrict__ keys, uint32_t n, uint32_t nt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t slot = tile_lookup(T, keys[i]);
  if (slot >= nt) return;
  P.updated[slot] = 1;
  P.dirty[slot] = 1;
}

}  // namespace ksk
