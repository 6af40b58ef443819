// ks_k_objects.h — semantic object instances from the device-resident map: the surface voxels of every label clustered into
// 26-connected components across tile seams, one integer record per component.  The contract (taking part, connectivity, the
// record, the order, the per-voxel ids) is DESIGN.md, section "Object instances"; tests/objects_model.py restates it in NumPy
// and the kernels are compared with it byte for byte.
//
// A voxel's GLOBAL ID is slot * 512 + local (local = x + 8 * (y + 8 * z), as everywhere); kObjNone = no voxel / no object.
// `parent` holds one word per voxel of the resident tiles: a union-find forest in which a link always points at a SMALLER id,
// so a root is the smallest id of its set whatever order the links were made in.
//
//   k_obj_label     one workgroup per tile, one work-item per voxel: the class byte (label, or kObjNoClass) from dwords 0..3
//                   of the record, a union-find over the 13 forward in-tile neighbours in LDS (32-bit LDS compare-and-swap),
//                   parent[id] = id of the in-tile root, or kObjNone
//   k_obj_seams     one workgroup per tile: the slots of the 13 forward neighbour TILES into LDS (tile_lookup, once), then every
//                   voxel on the tile's skin joins its set with those of its neighbours in these tiles: find both roots, CAS
//                   the larger root onto the smaller, until they are equal.  No work-item waits for another; the sets do not
//                   depend on the order of the atomics.  Each crossing pair is seen from exactly one side (the tile whose
//                   neighbour lies forward).
//   k_obj_number    every voxel finds its root and stores it (flat forest); roots take a provisional number (wave_append)
//   k_obj_acc_init  the accumulators of the provisional components
//   k_obj_reduce    per (wavefront, component): count, box, sums and the smallest position of the lanes that share the
//                   component, reduced across the lanes first; ONE set of integer atomics per (wavefront, component)
//   k_obj_keys      per component: the sort key (its smallest pack_coord3 word; all-ones below min_voxels) and the totals
//   (the library's radix sort orders the keys: the objects come first, ascending)
//   k_obj_records   the 72-byte records in that order, and provisional number -> final index
//   k_obj_ids       the per-voxel id store
//   k_obj_download  host-layout blocks of ids;  k_obj_query  the id of the voxel that contains each world point
//
// A wavefront of the per-voxel kernels covers one z-layer of a tile (64 voxels: all x, all y), so what k_obj_reduce reduces
// are LOCAL coordinates: three 10-bit sums in one word, an occupancy mask per axis (the box), the smallest local position.
#pragma once
#include "ks_types.h"

namespace ksk {

constexpr uint32_t kObjNone = 0xffffffffu;
constexpr uint8_t kObjNoClass = 0xffu;
constexpr uint32_t kObjLabels = 21;

struct ObjParams {
  float min_weight, surface_distance;
  uint32_t label_mask, min_voxels;
  uint32_t nt;   // resident tiles
};

struct ObjCounters {
  uint32_t n_components, n_objects, largest, pad;
  unsigned long long voxels_surface, voxels_in_objects;
};

struct ObjAcc {   // 64 B per provisional component
  unsigned long long first;   // smallest pack_coord3 word of its voxels
  unsigned long long sum[3];  // (two's complement: the sums of negative indices wrap as int64 does)
  int32_t bb_min[3], bb_max[3];
  uint32_t n, label;
};

static_assert(sizeof(ks_object) == 72 && sizeof(ObjAcc) == 64, "record layouts");

__device__ __forceinline__ uint32_t obj_local(int x, int y, int z) { return (uint32_t)x + 8u * ((uint32_t)y + 8u * (uint32_t)z); }

// ---- in-tile labelling ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t obj_find_lds(uint32_t* par, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ void obj_union_lds(uint32_t* par, uint32_t a, uint32_t b) {
  for (;;) {
    a = obj_find_lds(par, a);
    b = obj_find_lds(par, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(&par[a], a, b) == a) return;   // (a was still a root: linked; else someone linked it meanwhile: again)
  }
}

// grid (nt), 512 work-items
__global__ void __launch_bounds__(512) k_obj_label(Pool P, ObjParams O, uint8_t* __restrict__ cls_out, uint32_t* __restrict__ parent,
                                                   ObjCounters* __restrict__ C) {
  __shared__ uint8_t s_cls[kTileVoxels];
  __shared__ uint32_t s_par[kTileVoxels];
  const uint32_t slot = blockIdx.x, v = threadIdx.x;
  const size_t id = (size_t)slot * kTileVoxels + v;
  const uint4 q = P.vox[id * 8];
  const float d = __uint_as_float(q.x), w = __uint_as_float(q.y);
  const uint32_t label = q.w == 255u ? 0u : q.w;
  const bool part = w >= O.min_weight && fabsf(d) <= O.surface_distance && label < kObjLabels && ((O.label_mask >> label) & 1u);
  const uint8_t cls = part ? (uint8_t)label : kObjNoClass;
  s_cls[v] = cls;
  s_par[v] = v;
  const unsigned long long m = __ballot(part);
  if (lane_id() == 0 && m) atomicAdd(&C->voxels_surface, (unsigned long long)__popcll(m));
  __syncthreads();
  if (part) {
    const int x = (int)(v & 7u), y = (int)((v >> 3) & 7u), z = (int)(v >> 6);
    for (int o = 14; o < 27; ++o) {   // the 13 offsets after (0, 0, 0) in (z, y, x) order
      const int nx = x + o % 3 - 1, ny = y + (o / 3) % 3 - 1, nz = z + o / 9 - 1;
      if ((unsigned)nx > 7u || (unsigned)ny > 7u || (unsigned)nz > 7u) continue;
      const uint32_t n = obj_local(nx, ny, nz);
      if (s_cls[n] == cls) obj_union_lds(s_par, v, n);
    }
  }
  __syncthreads();
  cls_out[id] = cls;
  parent[id] = part ? slot * (uint32_t)kTileVoxels + obj_find_lds(s_par, v) : kObjNone;
}

// ---- seams -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t obj_find(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ void obj_union(uint32_t* parent, uint32_t a0, uint32_t b0) {
  uint32_t a = a0, b = b0;
  for (;;) {
    a = obj_find(parent, a);
    b = obj_find(parent, b);
    if (a == b) break;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(&parent[a], a, b) == a) break;
  }
  // shorten both paths: a link only ever moves to a smaller member of the same set, so this cannot undo anyone's link
  const uint32_t r = a < b ? a : b;
  if (r < a0) atomicMin(&parent[a0], r);
  if (r < b0) atomicMin(&parent[b0], r);
}

// grid (nt), 512 work-items.  s_nb[o]: the slot of the tile at offset o (as above: o = dx + 1 + 3 * (dy + 1) + 9 * (dz + 1)) for
// the forward offsets o > 13, kObjNone where no tile is resident.
__global__ void __launch_bounds__(512) k_obj_seams(TileTable T, ObjParams O, const uint8_t* __restrict__ cls, uint32_t* parent) {
  __shared__ uint32_t s_nb[27];
  const uint32_t slot = blockIdx.x, v = threadIdx.x;
  if (v < 27u) {
    uint32_t s = kObjNone;
    if (v > 13u) {
      int tx, ty, tz;
      unpack_tile(T.slot_keys[slot], tx, ty, tz);
      tx += (int)(v % 3u) - 1, ty += (int)((v / 3u) % 3u) - 1, tz += (int)(v / 9u) - 1;
      if (tx >= -kTileBias && tx < kTileBias && ty >= -kTileBias && ty < kTileBias && tz >= -kTileBias && tz < kTileBias) {
        s = tile_lookup(T, pack_tile(tx, ty, tz));
        if (s >= O.nt) s = kObjNone;
      }
    }
    s_nb[v] = s;
  }
  __syncthreads();
  const int x = (int)(v & 7u), y = (int)((v >> 3) & 7u), z = (int)(v >> 6);
  const bool skin = x == 0 || x == 7 || y == 0 || y == 7 || z == 0 || z == 7;
  const uint32_t id = slot * (uint32_t)kTileVoxels + v;
  const uint8_t c = cls[id];
  if (!skin || c == kObjNoClass) return;
  for (int o = 0; o < 27; ++o) {
    const int nx = x + o % 3 - 1, ny = y + (o / 3) % 3 - 1, nz = z + o / 9 - 1;
    const int t = (nx < 0 ? 0 : nx > 7 ? 2 : 1) + 3 * (ny < 0 ? 0 : ny > 7 ? 2 : 1) + 9 * (nz < 0 ? 0 : nz > 7 ? 2 : 1);
    if (t <= 13) continue;   // inside this tile (k_obj_label), or in a backward tile (that tile's work)
    const uint32_t ns = s_nb[t];
    if (ns == kObjNone) continue;
    const uint32_t n = ns * (uint32_t)kTileVoxels + obj_local(nx & 7, ny & 7, nz & 7);
    if (cls[n] == c) obj_union(parent, id, n);
  }
}

// ---- flatten and number ------------------------------------------------------------------------------------------------------
// grid (nt * 2), 256 work-items.  prov[root] = the provisional number of the root's component.
__global__ void __launch_bounds__(256) k_obj_number(uint32_t* parent, uint32_t* __restrict__ prov, ObjCounters* __restrict__ C) {
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  uint32_t r = kObjNone;
  if (__hip_atomic_load(&parent[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kObjNone) {
    r = obj_find(parent, id);
    // (another work-item may be walking through this voxel: it reads the old link or the root, both lead to the root)
    if (r != id) __hip_atomic_store(&parent[id], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const uint32_t n = wave_append(r == id, &C->n_components);
  if (r == id) prov[id] = n;
}

__global__ void __launch_bounds__(256) k_obj_acc_init(ObjAcc* __restrict__ acc, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  ObjAcc a;
  a.first = ~0ull;
  for (int k = 0; k < 3; ++k) a.sum[k] = 0ull, a.bb_min[k] = 0x7fffffff, a.bb_max[k] = (int32_t)0x80000000u;
  a.n = 0u;
  a.label = 0u;
  acc[i] = a;
}

// ---- reduce -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t obj_wave_add(uint32_t v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint32_t obj_wave_or(uint32_t v) {
  for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint32_t obj_wave_min(uint32_t v) {
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t u = __shfl_xor(v, o);
    v = u < v ? u : v;
  }
  return v;
}

// grid (nt * 2), 256 work-items: a wavefront is the z-layer (id >> 6) & 7 of tile id >> 9.  parent[id] becomes the voxel's
// provisional component number (its link is not needed again: every other work-item reads its OWN link, and prov of a root).
__global__ void __launch_bounds__(256) k_obj_reduce(TileTable T, const uint8_t* __restrict__ cls, uint32_t* parent, const uint32_t* __restrict__ prov,
                                                    ObjAcc* __restrict__ acc) {
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = lane_id();
  const uint32_t root = parent[id];
  const uint32_t comp = root == kObjNone ? kObjNone : prov[root];
  parent[id] = comp;
  unsigned long long left = __ballot(comp != kObjNone);
  if (!left) return;   // (uniform)
  int tx, ty, tz;
  unpack_tile(T.slot_keys[id >> 9], tx, ty, tz);
  const int lx = (int)(id & 7u), ly = (int)((id >> 3) & 7u), lz = (int)((id >> 6) & 7u);
  while (left) {
    const int leader = __ffsll((long long)left) - 1;
    const uint32_t c = __shfl(comp, leader);
    const bool mine = comp == c;
    const unsigned long long m = __ballot(mine);
    const uint32_t sums = obj_wave_add(mine ? (uint32_t)lx | ((uint32_t)ly << 10) | ((uint32_t)lz << 20) : 0u);
    const uint32_t occ = obj_wave_or(mine ? (1u << lx) | (1u << (8 + ly)) | (1u << (16 + lz)) : 0u);
    const uint32_t low = obj_wave_min(mine ? ((uint32_t)lx << 6) | ((uint32_t)ly << 3) | (uint32_t)lz : kObjNone);
    if ((int)lane == leader) {
      ObjAcc* A = acc + c;
      const uint32_t n = (uint32_t)__popcll(m);
      const int base[3] = {8 * tx, 8 * ty, 8 * tz};
      const uint32_t s[3] = {sums & 1023u, (sums >> 10) & 1023u, sums >> 20};
      atomicAdd(&A->n, n);
      for (int k = 0; k < 3; ++k) {
        const uint32_t ok = (occ >> (8 * k)) & 255u;
        atomicMin(&A->bb_min[k], base[k] + __ffs((int)ok) - 1);
        atomicMax(&A->bb_max[k], base[k] + 31 - __clz((int)ok));
        atomicAdd(&A->sum[k], (unsigned long long)((long long)n * (long long)base[k] + (long long)s[k]));
      }
      atomicMin(&A->first, (unsigned long long)pack_coord3(base[0] + (int)(low >> 6), base[1] + (int)((low >> 3) & 7u), base[2] + (int)(low & 7u)));
      A->label = (uint32_t)cls[id];   // (every writer stores the same value)
    }
    left &= ~m;
  }
}

// ---- filter, order, assign -----------------------------------------------------------------------------------------------------
// One lane per provisional component.  A component below min_voxels gets the all-ones key: it sorts behind every object.
__global__ void __launch_bounds__(256) k_obj_keys(const ObjAcc* __restrict__ acc, uint32_t n, uint32_t min_voxels, uint64_t* __restrict__ keys,
                                                  uint32_t* __restrict__ vals, ObjCounters* __restrict__ C) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t nv = 0;
  if (i < n) {
    const uint32_t a = acc[i].n;
    const bool object = a >= min_voxels;
    keys[i] = object ? (uint64_t)acc[i].first : ~0ull;
    vals[i] = i;
    nv = object ? a : 0u;
  }
  const unsigned long long m = __ballot(nv != 0u);
  const uint32_t total = obj_wave_add(nv);
  uint32_t big = nv;
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t u = __shfl_xor(big, o);
    big = u > big ? u : big;
  }
  if (lane_id() == 0 && m) {
    atomicAdd(&C->n_objects, (uint32_t)__popcll(m));
    atomicAdd(&C->voxels_in_objects, (unsigned long long)total);
    atomicMax(&C->largest, big);
  }
}

// One lane per sorted position: position i < number of objects is object i.
__global__ void __launch_bounds__(256) k_obj_records(const ObjAcc* __restrict__ acc, uint32_t n, const uint64_t* __restrict__ keys,
                                                     const uint32_t* __restrict__ vals, ks_object* __restrict__ rec, uint32_t* __restrict__ final_of) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = vals[i];
  if (keys[i] == ~0ull) {
    final_of[c] = kObjNone;
    return;
  }
  final_of[c] = i;
  const ObjAcc a = acc[c];
  ks_object r;
  unpack_coord3((uint64_t)a.first, r.first_voxel[0], r.first_voxel[1], r.first_voxel[2]);
  r.n_voxels = a.n;
  for (int k = 0; k < 3; ++k) r.bb_min[k] = a.bb_min[k], r.bb_max[k] = a.bb_max[k], r.sum[k] = (int64_t)a.sum[k];
  r.label = a.label;
  r.pad = 0u;
  rec[i] = r;
}

// parent holds the provisional numbers (k_obj_reduce)
__global__ void __launch_bounds__(256) k_obj_ids(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ final_of, uint32_t* __restrict__ ids,
                                                 size_t n) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = parent[i];
  ids[i] = c == kObjNone ? kObjNone : final_of[c];
}

// ---- readers of the id store (the layouts and rules of k_esdf_download / k_esdf_query) ---------------------------------------
__global__ void __launch_bounds__(256) k_obj_download(TileTable T, const uint32_t* __restrict__ ids, uint32_t n_tiles,
                                                      const int32_t* __restrict__ block_idx, int vps, uint32_t* __restrict__ out) {
  const uint32_t b = blockIdx.y;
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nv = (uint32_t)(vps * vps * vps);
  if (l >= nv) return;
  const int lx = (int)(l % (uint32_t)vps), ly = (int)((l / (uint32_t)vps) % (uint32_t)vps), lz = (int)(l / (uint32_t)(vps * vps));
  const int64_t vx = (int64_t)block_idx[3 * b] * vps + lx, vy = (int64_t)block_idx[3 * b + 1] * vps + ly, vz = (int64_t)block_idx[3 * b + 2] * vps + lz;
  uint32_t id = kObjNone;
  const int64_t tx = vx >> 3, ty = vy >> 3, tz = vz >> 3;
  if (tx >= -kTileBias && tx < kTileBias && ty >= -kTileBias && ty < kTileBias && tz >= -kTileBias && tz < kTileBias) {
    const uint32_t slot = tile_lookup(T, pack_tile((int)tx, (int)ty, (int)tz));
    if (slot < n_tiles) id = ids[(size_t)slot * kTileVoxels + obj_local((int)(vx & 7), (int)(vy & 7), (int)(vz & 7))];
  }
  out[(size_t)b * nv + l] = id;
}

__global__ void __launch_bounds__(256) k_obj_query(TileTable T, const uint32_t* __restrict__ ids, uint32_t n_tiles, const float* __restrict__ xyz,
                                                   size_t n, float voxel_size_inv, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float gx = grid_coord(xyz[3 * i], voxel_size_inv), gy = grid_coord(xyz[3 * i + 1], voxel_size_inv),
              gz = grid_coord(xyz[3 * i + 2], voxel_size_inv);
  uint32_t id = kObjNone;
  const float lim = (float)(kCoordBias - 1);
  if (fabsf(gx) < lim && fabsf(gy) < lim && fabsf(gz) < lim) {
    const int vx = (int)gx, vy = (int)gy, vz = (int)gz;
    const uint32_t slot = tile_lookup(T, pack_tile(vx >> 3, vy >> 3, vz >> 3));
    if (slot < n_tiles) id = ids[(size_t)slot * kTileVoxels + obj_local(vx & 7, vy & 7, vz & 7)];
  }
  out[i] = id;
}

}  // namespace ksk
