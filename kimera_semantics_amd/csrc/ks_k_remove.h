// ks_k_remove.h — taking tiles out of the resident map (ks_remove_blocks, ks_remove_distant_blocks).
//   k_remove_select_list      one lane per tile key of the listed blocks: the key's slot, if it has one, is marked
//   k_remove_select_distance  one lane per slot: the rule of Voxblox's Layer::removeDistantBlocks on the slot's BLOCK
//   k_remove_move             one workgroup per moved tile: the 64 KiB record block, the key, the four flags, the stored
//                             ESDF records and object ids go from a slot at or above the new tile count into a hole below it
// The holes and the tail survivors are paired on the host (a linear walk over the byte plane it has to read anyway: the
// stored products' bookkeeping needs the keys of what left); sources and destinations are disjoint, so the moves need no
// order.  The directory is rebuilt afterwards by k_rehash_tiles (ks_k_io.h) — the sequence of grow_pool.
#pragma once
#include "ks_k_esdf.h"
#include "ks_types.h"

namespace ksk {

__global__ void __launch_bounds__(256) k_remove_select_list(TileTable T, const uint64_t* __restrict__ keys, uint32_t n, uint32_t nt,
                                                            uint8_t* __restrict__ remove) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t slot = tile_lookup(T, keys[i]);
  if (slot < nt) remove[slot] = 1;   // (a block listed twice stores the same byte twice)
}

// The block goes iff d2 > max_distance^2 with, in f32 and in this order (the library is built without contraction):
//   block_size = voxel_size * (float)vps;  o_k = (float)b_k * block_size;  d_k = o_k - center_k;  d2 = (dx dx + dy dy) + dz dz.
// Every tile of a block evaluates the same block index, so a block leaves whole.
struct RemoveRule {
  float block_size, cx, cy, cz, max_distance;
  int vps_shift;
};
__device__ __forceinline__ bool remove_rule(const RemoveRule& R, int bx, int by, int bz) {
  const float ox = (float)bx * R.block_size, oy = (float)by * R.block_size, oz = (float)bz * R.block_size;
  const float dx = ox - R.cx, dy = oy - R.cy, dz = oz - R.cz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float d2 = (xx + yy) + zz;
  const float m2 = R.max_distance * R.max_distance;
  return d2 > m2;
}
__global__ void __launch_bounds__(256) k_remove_select_distance(const uint64_t* __restrict__ slot_keys, uint32_t nt, RemoveRule R,
                                                                uint8_t* __restrict__ remove) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nt) return;
  int tx, ty, tz;
  unpack_tile(slot_keys[slot], tx, ty, tz);
  remove[slot] = remove_rule(R, tx >> R.vps_shift, ty >> R.vps_shift, tz >> R.vps_shift) ? 1 : 0;
}

// moves[i] = {source slot, destination slot}.  esdf / obj_ids: the per-slot stores (nullptr: none is stored), valid for slots
// below esdf_tiles / obj_tiles.  A tile that joined the map after a store was made has no records in it: where its
// destination lies inside the store it gets default records there, and the ESDF's stale bit, which the refresh reads.
__global__ void __launch_bounds__(512) k_remove_move(Pool P, uint64_t* __restrict__ slot_keys, const uint2* __restrict__ moves,
                                                     EsdfRecord* __restrict__ esdf, uint32_t esdf_tiles, uint32_t* __restrict__ obj_ids,
                                                     uint32_t obj_tiles) {
  const uint32_t src = moves[blockIdx.x].x, dst = moves[blockIdx.x].y;
  const uint4* from = P.vox + (size_t)src * kTileVoxels * 8;
  uint4* to = P.vox + (size_t)dst * kTileVoxels * 8;
  uint4 v[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = from[r * 512 + threadIdx.x];
#pragma unroll
  for (int r = 0; r < 8; ++r) to[r * 512 + threadIdx.x] = v[r];
  const bool esdf_fresh = esdf && dst < esdf_tiles && src >= esdf_tiles;
  if (esdf && dst < esdf_tiles)
    esdf[(size_t)dst * kTileVoxels + threadIdx.x] = esdf_fresh ? EsdfRecord{0.0f, kEsdfDefaultTail} : esdf[(size_t)src * kTileVoxels + threadIdx.x];
  if (obj_ids && dst < obj_tiles)
    obj_ids[(size_t)dst * kTileVoxels + threadIdx.x] = src < obj_tiles ? obj_ids[(size_t)src * kTileVoxels + threadIdx.x] : KS_OBJECT_NONE;
  if (threadIdx.x == 0) {
    slot_keys[dst] = slot_keys[src];
    P.updated[dst] = P.updated[src];
    P.dirty[dst] = P.dirty[src];
    P.mesh_stale()[dst] = (uint8_t)(P.mesh_stale()[src] | (esdf_fresh ? kStaleEsdf : 0));
  }
}

}  // namespace ksk
