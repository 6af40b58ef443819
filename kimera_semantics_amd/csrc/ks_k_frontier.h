// ks_k_frontier.h — exploration frontiers over the stored ESDF: the traversable voxels with an unobserved face neighbour,
// clustered into 26-connected components across tile seams, one integer record per component, joined with the navigation field.
// The contract (observed, traversable, frontier voxel, bounds, the record, the join, the order, the per-voxel ids) is DESIGN.md,
// section "Exploration frontiers"; tests/frontier_model.py restates it in NumPy and the kernels are compared with it byte for byte.
// The ESDF store and the navigation field are only read.
//
// A wavefront of the per-voxel kernels covers one z-layer of a tile (64 voxels: all x, all y; lane = x + 8 * y), so a layer of
// one-bit facts is ONE 64-bit ballot.  After pass 1 a tile is 16 such words (128 B): planes[slot * 16 + 2 * z] = observed,
// planes[slot * 16 + 2 * z + 1] = candidate (traversable and inside the bounds).  No later pass touches the records.
//
//   k_fr_planes    a lane per voxel of the store's tiles: one 8-byte load of the record, two ballots, two stores per wavefront
//   k_fr_classify  one workgroup per tile: the slots of the six face-neighbour tiles (tile_lookup, once), the own planes and the
//                  neighbours' observed planes into LDS (an absent tile reads all-zero: nothing observed); every lane tests the
//                  six observed bits around it (+-x, +-y: bits of its own or the neighbour tile's layer word; +-z: the adjacent
//                  layers), writes the class byte (kFrClass or kObjNoClass) and its unknown-face count, and the frontier voxels
//                  run k_obj_label's in-tile union-find in LDS
//   (k_obj_seams, k_obj_number of ks_k_objects.h as they are, with frontier as the one class: seams, flat forest, numbers)
//   k_fr_acc_init  the accumulators of the provisional components
//   k_fr_reduce    k_obj_reduce plus, per (wavefront, component), the sum of the unknown faces (u32 add) and the smallest
//                  reached cost of the navigation field (u32 min): pass one of the join
//   k_fr_nav_pick  pass two of the join: among the voxels AT the component's smallest cost, the smallest pack_coord3 word
//                  (u64 min).  Nothing in either pass knows a slot number, so the result does not depend on the block order.
//   k_fr_keys      per component: the sort key (its smallest pack_coord3 word; all-ones below min_voxels) and the totals
//   (the library's radix sort orders the keys)
//   k_fr_records   the 88-byte records in that order, and provisional number -> final index
//   (k_obj_ids; k_obj_download and k_obj_query read the id store: kFrNone == kObjNone)
// Integer atomics only.
#pragma once
#include "ks_k_nav.h"

namespace ksk {

constexpr uint32_t kFrNone = KS_FRONTIER_NONE;
constexpr uint8_t kFrClass = 0;   // the one class k_obj_seams sees
static_assert(kFrNone == kObjNone, "the id store is read by k_obj_download and k_obj_query");

struct FrParams {
  float radius;
  uint32_t min_voxels;
  int32_t use_bounds;
  int32_t bmin[3], bmax[3];
  uint32_t nt;   // tiles of the ESDF store
};

struct FrCounters {   // 64 B
  unsigned long long traversable, frontier_voxels, unknown_faces, voxels_in_frontiers;
  uint32_t n_frontiers, largest;
  uint32_t pad[6];
};

struct FrAcc {   // 80 B per provisional component
  unsigned long long first;     // smallest pack_coord3 word of its voxels
  unsigned long long sum[3];    // (two's complement, as ObjAcc)
  unsigned long long nav_key;   // smallest pack_coord3 word among the voxels at nav_cost
  int32_t bb_min[3], bb_max[3];
  uint32_t n, faces, nav_cost, pad;
};

static_assert(sizeof(ks_frontier) == 88 && sizeof(FrAcc) == 80 && sizeof(FrCounters) == 64, "record layouts");
static_assert(sizeof(ks_frontier_config) == 40 && sizeof(ks_frontier_stats) == 72, "ABI");

// ---- pass 1: the bit planes -----------------------------------------------------------------------------------------------
// grid (nt * 2), 256 work-items: a wavefront is the z-layer (id >> 6) & 7 of tile id >> 9
__global__ void __launch_bounds__(256) k_fr_planes(TileTable T, FrParams F, const EsdfRecord* __restrict__ store,
                                                   unsigned long long* __restrict__ planes, FrCounters* __restrict__ C) {
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  const EsdfRecord r = store[id];
  const bool observed = (r.tail & 1u) != 0u;
  const bool traversable = observed && r.distance >= F.radius;   // (a NaN distance is not traversable)
  bool candidate = traversable;
  if (F.use_bounds) {   // (uniform)
    int tx, ty, tz;
    unpack_tile(T.slot_keys[id >> 9], tx, ty, tz);
    const int gx = 8 * tx + (int)(id & 7u), gy = 8 * ty + (int)((id >> 3) & 7u), gz = 8 * tz + (int)((id >> 6) & 7u);
    candidate = traversable && gx >= F.bmin[0] && gx <= F.bmax[0] && gy >= F.bmin[1] && gy <= F.bmax[1] && gz >= F.bmin[2] && gz <= F.bmax[2];
  }
  const unsigned long long mo = __ballot(observed), mc = __ballot(candidate), mt = __ballot(traversable);
  const uint32_t lane = lane_id();
  if (lane < 2u) planes[(size_t)(id >> 6) * 2u + lane] = lane ? mc : mo;
  if (lane == 0 && mt) atomicAdd(&C->traversable, (unsigned long long)__popcll(mt));
}

// ---- classification and in-tile labelling ------------------------------------------------------------------------------------
// grid (nt), 512 work-items.  s_nb[d]: the slot of the face-neighbour tile in direction d = 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z.
__global__ void __launch_bounds__(512) k_fr_classify(TileTable T, FrParams F, const unsigned long long* __restrict__ planes,
                                                     uint8_t* __restrict__ cls_out, uint8_t* __restrict__ faces_out, uint32_t* __restrict__ parent,
                                                     FrCounters* __restrict__ C) {
  __shared__ uint32_t s_nb[6];
  __shared__ unsigned long long s_own[16];      // [z][observed | candidate]
  __shared__ unsigned long long s_nobs[6][8];   // the observed layers of the six neighbours
  __shared__ uint8_t s_cls[kTileVoxels];
  __shared__ uint32_t s_par[kTileVoxels];
  const uint32_t slot = blockIdx.x, v = threadIdx.x;
  if (v < 6u) {
    int t[3];
    unpack_tile(T.slot_keys[slot], t[0], t[1], t[2]);
    t[v >> 1] += (v & 1u) ? 1 : -1;
    uint32_t s = kObjNone;
    if (t[0] >= -kTileBias && t[0] < kTileBias && t[1] >= -kTileBias && t[1] < kTileBias && t[2] >= -kTileBias && t[2] < kTileBias) {
      s = tile_lookup(T, pack_tile(t[0], t[1], t[2]));
      if (s >= F.nt) s = kObjNone;   // (a tile that joined after the store was made: unknown)
    }
    s_nb[v] = s;
  }
  if (v >= 64u && v < 80u) s_own[v - 64u] = planes[(size_t)slot * 16u + (v - 64u)];
  __syncthreads();
  if (v < 48u) {
    const uint32_t ns = s_nb[v >> 3];
    s_nobs[v >> 3][v & 7u] = ns == kObjNone ? 0ull : planes[(size_t)ns * 16u + 2u * (v & 7u)];
  }
  s_par[v] = v;
  __syncthreads();
  const int x = (int)(v & 7u), y = (int)((v >> 3) & 7u), z = (int)(v >> 6);
  const uint32_t b = v & 63u;
  const unsigned long long own = s_own[2 * z];
  const bool candidate = ((s_own[2 * z + 1] >> b) & 1ull) != 0ull;
  uint32_t seen = 0;
  seen += (uint32_t)((x > 0 ? own >> (b - 1u) : s_nobs[0][z] >> (b + 7u)) & 1ull);
  seen += (uint32_t)((x < 7 ? own >> (b + 1u) : s_nobs[1][z] >> (b - 7u)) & 1ull);
  seen += (uint32_t)((y > 0 ? own >> (b - 8u) : s_nobs[2][z] >> (b + 56u)) & 1ull);
  seen += (uint32_t)((y < 7 ? own >> (b + 8u) : s_nobs[3][z] >> (b - 56u)) & 1ull);
  seen += (uint32_t)(((z > 0 ? s_own[2 * z - 2] : s_nobs[4][7]) >> b) & 1ull);
  seen += (uint32_t)(((z < 7 ? s_own[2 * z + 2] : s_nobs[5][0]) >> b) & 1ull);
  const uint32_t unknown = 6u - seen;
  const bool part = candidate && unknown != 0u;
  const uint8_t cls = part ? kFrClass : kObjNoClass;
  s_cls[v] = cls;
  const unsigned long long m = __ballot(part);
  const uint32_t faces = obj_wave_add(part ? unknown : 0u);
  if (lane_id() == 0 && m) {
    atomicAdd(&C->frontier_voxels, (unsigned long long)__popcll(m));
    atomicAdd(&C->unknown_faces, (unsigned long long)faces);
  }
  __syncthreads();
  if (part) {
    for (int o = 14; o < 27; ++o) {   // the 13 offsets after (0, 0, 0) in (z, y, x) order, as k_obj_label
      const int nx = x + o % 3 - 1, ny = y + (o / 3) % 3 - 1, nz = z + o / 9 - 1;
      if ((unsigned)nx > 7u || (unsigned)ny > 7u || (unsigned)nz > 7u) continue;
      const uint32_t n = obj_local(nx, ny, nz);
      if (s_cls[n] == cls) obj_union_lds(s_par, v, n);
    }
  }
  __syncthreads();
  const size_t id = (size_t)slot * kTileVoxels + v;
  cls_out[id] = cls;
  faces_out[id] = part ? (uint8_t)unknown : (uint8_t)0;
  parent[id] = part ? slot * (uint32_t)kTileVoxels + obj_find_lds(s_par, v) : kObjNone;
}

__global__ void __launch_bounds__(256) k_fr_acc_init(FrAcc* __restrict__ acc, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  FrAcc a;
  a.first = ~0ull;
  a.nav_key = ~0ull;
  for (int k = 0; k < 3; ++k) a.sum[k] = 0ull, a.bb_min[k] = 0x7fffffff, a.bb_max[k] = (int32_t)0x80000000u;
  a.n = 0u;
  a.faces = 0u;
  a.nav_cost = kNavUnreached;
  a.pad = 0u;
  acc[i] = a;
}

// ---- reduce ---------------------------------------------------------------------------------------------------------------
// grid (nt * 2), 256 work-items, a wavefront per z-layer of a tile as in k_obj_reduce.  parent[id] becomes the voxel's provisional
// component number.  field: the navigation field over the same slots, or nullptr.
__global__ void __launch_bounds__(256) k_fr_reduce(TileTable T, const uint8_t* __restrict__ faces, const uint32_t* __restrict__ field, uint32_t* parent,
                                                   const uint32_t* __restrict__ prov, FrAcc* __restrict__ acc) {
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = lane_id();
  const uint32_t root = parent[id];
  const uint32_t comp = root == kObjNone ? kObjNone : prov[root];
  parent[id] = comp;
  unsigned long long left = __ballot(comp != kObjNone);
  if (!left) return;   // (uniform)
  uint32_t nf = 0u, cost = kNavUnreached;
  if (comp != kObjNone) {
    nf = (uint32_t)faces[id];
    if (field) {
      const uint32_t f = field[id];
      if (f <= kNavMaxCost) cost = f;
    }
  }
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
    const uint32_t fsum = obj_wave_add(mine ? nf : 0u);
    const uint32_t cmin = obj_wave_min(mine ? cost : kNavUnreached);
    if ((int)lane == leader) {
      FrAcc* A = acc + c;
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
      atomicAdd(&A->faces, fsum);
      if (cmin != kNavUnreached) atomicMin(&A->nav_cost, cmin);
    }
    left &= ~m;
  }
}

// grid (nt * 2), 256 work-items.  parent holds the provisional numbers, acc[].nav_cost is final (k_fr_reduce has completed).
__global__ void __launch_bounds__(256) k_fr_nav_pick(TileTable T, const uint32_t* __restrict__ field, const uint32_t* __restrict__ parent,
                                                     FrAcc* __restrict__ acc) {
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = lane_id();
  const uint32_t comp = parent[id];
  bool hit = false;
  if (comp != kObjNone) {
    const uint32_t best = acc[comp].nav_cost;
    hit = best != kNavUnreached && field[id] == best;
  }
  unsigned long long left = __ballot(hit);
  if (!left) return;   // (uniform)
  int tx, ty, tz;
  unpack_tile(T.slot_keys[id >> 9], tx, ty, tz);
  const int lx = (int)(id & 7u), ly = (int)((id >> 3) & 7u), lz = (int)((id >> 6) & 7u);
  while (left) {
    const int leader = __ffsll((long long)left) - 1;
    const uint32_t c = __shfl(comp, leader);
    const bool mine = hit && comp == c;
    const unsigned long long m = __ballot(mine);
    const uint32_t low = obj_wave_min(mine ? ((uint32_t)lx << 6) | ((uint32_t)ly << 3) | (uint32_t)lz : kObjNone);
    if ((int)lane == leader)
      atomicMin(&acc[c].nav_key, (unsigned long long)pack_coord3(8 * tx + (int)(low >> 6), 8 * ty + (int)((low >> 3) & 7u), 8 * tz + (int)(low & 7u)));
    left &= ~m;
  }
}

// ---- filter, order, assign -------------------------------------------------------------------------------------------------
// One lane per provisional component.  A component below min_voxels gets the all-ones key: it sorts behind every frontier.
__global__ void __launch_bounds__(256) k_fr_keys(const FrAcc* __restrict__ acc, uint32_t n, uint32_t min_voxels, uint64_t* __restrict__ keys,
                                                 uint32_t* __restrict__ vals, FrCounters* __restrict__ C) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t nv = 0;
  if (i < n) {
    const uint32_t a = acc[i].n;
    const bool frontier = a >= min_voxels;
    keys[i] = frontier ? (uint64_t)acc[i].first : ~0ull;
    vals[i] = i;
    nv = frontier ? a : 0u;
  }
  const unsigned long long m = __ballot(nv != 0u);
  const uint32_t total = obj_wave_add(nv);
  uint32_t big = nv;
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t u = __shfl_xor(big, o);
    big = u > big ? u : big;
  }
  if (lane_id() == 0 && m) {
    atomicAdd(&C->n_frontiers, (uint32_t)__popcll(m));
    atomicAdd(&C->voxels_in_frontiers, (unsigned long long)total);
    atomicMax(&C->largest, big);
  }
}

// One lane per sorted position: position i < number of frontiers is frontier i.
__global__ void __launch_bounds__(256) k_fr_records(const FrAcc* __restrict__ acc, uint32_t n, const uint64_t* __restrict__ keys,
                                                    const uint32_t* __restrict__ vals, ks_frontier* __restrict__ rec, uint32_t* __restrict__ final_of) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = vals[i];
  if (keys[i] == ~0ull) {
    final_of[c] = kObjNone;
    return;
  }
  final_of[c] = i;
  const FrAcc a = acc[c];
  ks_frontier r;
  unpack_coord3((uint64_t)a.first, r.first_voxel[0], r.first_voxel[1], r.first_voxel[2]);
  r.n_voxels = a.n;
  for (int k = 0; k < 3; ++k) r.bb_min[k] = a.bb_min[k], r.bb_max[k] = a.bb_max[k], r.sum[k] = (int64_t)a.sum[k];
  r.unknown_faces = a.faces;
  r.nav_cost = a.nav_cost;
  unpack_coord3((uint64_t)(a.nav_cost == kNavUnreached ? a.first : a.nav_key), r.nav_voxel[0], r.nav_voxel[1], r.nav_voxel[2]);
  r.pad = 0u;
  rec[i] = r;
}

}  // namespace ksk
