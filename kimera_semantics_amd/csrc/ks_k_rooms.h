// ks_k_rooms.h — rooms over the stored ESDF: the free voxels whose stored distance reaches core_distance_m clustered into
// 26-connected components across tile seams (the cores: free space falls apart where it gets narrow), every other free voxel handed
// to the room that is nearest through free space, the contacts between rooms sorted into links, the stored objects joined.
// The contract (free, core, room, growth, the records, the links, the join, the order, the two per-voxel planes) is DESIGN.md,
// section "Rooms"; tests/rooms_model.py restates it in NumPy and the kernels are compared with it byte for byte.  The ESDF store
// and the object ids are only read.
//
//   k_room_classify  one workgroup per tile: free and core from the 8-byte record (and the bounds); the class byte (kRoomClass or
//                    kObjNoClass), the initial cost (k_nav_init's rule with free_distance_m: kNavUnreached | kNavBlocked) and, for
//                    the core voxels, k_obj_label's in-tile union-find in LDS
//   (k_obj_seams, k_obj_number, k_obj_acc_init, k_obj_reduce, k_obj_keys, the radix sort, k_obj_records of ks_k_objects.h as they
//    are, with core as the one class and min_core_voxels as the filter: the rooms in their order, provisional number -> room)
//   k_room_seed      a wavefront per z-layer of a tile: the room plane (the room of a core voxel of a room, kRoomNone elsewhere),
//                    cost 0 on those cores, and their tiles on list 0, once each (the `queued` exchange of k_nav_seed); with
//                    write = 0 it only makes the list again, for the second relaxation
//   (k_nav_relax of ks_k_nav.h as it is: its fixed point from these seeds is the multi-source cost)
//   k_room_assign    one workgroup per ACTIVE tile, with the costs final: the 10 x 10 x 10 halos of cost (fixed) and room
//                    (decreasing) in LDS; room(v) = min(room(v), room(u)) over the neighbours u with cost(u) + w(u, v) == cost(v),
//                    in sweeps with one barrier each until nothing changes.  Every value ever stored is the index of a room that has a
//                    shortest path to v and values only decrease, so the fixed point is the smallest such index whatever a tile
//                    read of its neighbours and when.  Lists, `queued` and the three counts as in k_nav_relax.
//   k_room_reduce    per (wavefront, room): count, box, index sums and largest cost of the assigned voxels, the largest distance bits
//                    of the room's core voxels (u32 max: the bits of a non-negative finite float order as the floats do)
//   k_room_pick      pass two: among the core voxels AT the room's largest bits, the smallest pack_coord3 word (u64 min)
//   k_room_contacts  one workgroup per tile, the room halo in LDS: the (voxel, other room) incidences; mode 0 counts them, mode 1
//                    appends key a << 32 | b (a < b) with the voxel's id as payload.  Where a pair lands in the buffer depends on the
//                    schedule; nothing that is derived from a run of equal keys does (a count, a maximum, a minimum).
//   (the radix sort orders the pairs by key)
//   k_room_heads     the first pair of every run: (key, position) appended; (the radix sort orders the heads: link j starts at
//                    position starts[j] and ends where link j + 1 starts)
//   k_room_link_max / k_room_link_pick   the two-pass pick over the sorted pairs; a pair finds its link by bisection of starts
//   k_room_links     the 32-byte link records, and n_links of both rooms
//   k_room_obj_min   a lane per voxel both id stores cover: 64-bit atomicMin of cost << 32 | room per object
//   k_room_obj_join  a lane per object: its room, and n_objects of that room
//   k_room_records   the 96-byte records, and the totals
//   (k_obj_download and k_obj_query read both planes: kRoomNone == kObjNone == kNavBlocked)
// Integer atomics only; nothing wider than 32 bits travels between running workgroups.
#pragma once
#include "ks_k_nav.h"

namespace ksk {

constexpr uint32_t kRoomNone = KS_ROOM_NONE;
constexpr uint8_t kRoomClass = 0;   // the one class k_obj_seams sees
static_assert(kRoomNone == kObjNone && kRoomNone == kNavBlocked, "both planes are read by k_obj_download and k_obj_query");

struct RoomParams {
  float free_distance, core_distance;
  int32_t use_bounds;
  int32_t bmin[3], bmax[3];
  uint32_t nt;   // tiles of the ESDF store
};

struct RoomCounters {   // 64 B
  unsigned long long free_voxels, core_voxels, assigned, contacts;
  uint32_t largest_room, largest_cost, n_pairs, n_links, objects_joined, cursor /* where mode 1 of k_room_contacts appends */, pad[2];
};

struct RoomAcc {   // 80 B per room
  unsigned long long centre;    // smallest pack_coord3 word among the core voxels at `clearance`
  unsigned long long sum[3];    // (two's complement, as ObjAcc)
  int32_t bb_min[3], bb_max[3];
  uint32_t n, largest_cost, clearance, n_links, n_objects, pad;
};

struct RoomLinkAcc {   // 16 B per link
  unsigned long long door;   // smallest pack_coord3 word among the contacts at `clearance`
  uint32_t clearance, pad;
};

static_assert(sizeof(ks_room) == 96 && sizeof(ks_room_link) == 32 && sizeof(RoomAcc) == 80 && sizeof(RoomLinkAcc) == 16 && sizeof(RoomCounters) == 64,
              "record layouts");
static_assert(sizeof(ks_rooms_config) == 48 && sizeof(ks_rooms_stats) == 120, "ABI");

__device__ __forceinline__ uint32_t room_wave_max(uint32_t v) {
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return v;
}

// the global index of voxel id = slot * 512 + local
__device__ __forceinline__ void room_voxel_of(const TileTable& T, uint32_t id, int& gx, int& gy, int& gz) {
  int tx, ty, tz;
  unpack_tile(T.slot_keys[id >> 9], tx, ty, tz);
  gx = 8 * tx + (int)(id & 7u), gy = 8 * ty + (int)((id >> 3) & 7u), gz = 8 * tz + (int)((id >> 6) & 7u);
}

// ---- classes, initial costs and the in-tile forest --------------------------------------------------------------------------
// grid (nt), 512 work-items
__global__ void __launch_bounds__(512) k_room_classify(TileTable T, RoomParams R, const EsdfRecord* __restrict__ store, uint8_t* __restrict__ cls_out,
                                                       uint32_t* __restrict__ parent, uint32_t* __restrict__ cost, RoomCounters* __restrict__ C) {
  __shared__ uint8_t s_cls[kTileVoxels];
  __shared__ uint32_t s_par[kTileVoxels];
  const uint32_t slot = blockIdx.x, v = threadIdx.x;
  const size_t id = (size_t)slot * kTileVoxels + v;
  const EsdfRecord r = store[id];
  const int x = (int)(v & 7u), y = (int)((v >> 3) & 7u), z = (int)(v >> 6);
  bool is_free = (r.tail & 1u) != 0u && r.distance >= R.free_distance;   // (a NaN distance is not free)
  if (R.use_bounds) {   // (uniform)
    int tx, ty, tz;
    unpack_tile(T.slot_keys[slot], tx, ty, tz);
    const int gx = 8 * tx + x, gy = 8 * ty + y, gz = 8 * tz + z;
    is_free = is_free && gx >= R.bmin[0] && gx <= R.bmax[0] && gy >= R.bmin[1] && gy <= R.bmax[1] && gz >= R.bmin[2] && gz <= R.bmax[2];
  }
  const bool core = is_free && r.distance >= R.core_distance;
  const uint8_t cls = core ? kRoomClass : kObjNoClass;
  s_cls[v] = cls;
  s_par[v] = v;
  const unsigned long long mf = __ballot(is_free), mc = __ballot(core);
  if (lane_id() == 0) {
    if (mf) atomicAdd(&C->free_voxels, (unsigned long long)__popcll(mf));
    if (mc) atomicAdd(&C->core_voxels, (unsigned long long)__popcll(mc));
  }
  __syncthreads();
  if (core) {
    for (int o = 14; o < 27; ++o) {   // the 13 offsets after (0, 0, 0) in (z, y, x) order, as k_obj_label
      const int nx = x + o % 3 - 1, ny = y + (o / 3) % 3 - 1, nz = z + o / 9 - 1;
      if ((unsigned)nx > 7u || (unsigned)ny > 7u || (unsigned)nz > 7u) continue;
      const uint32_t n = obj_local(nx, ny, nz);
      if (s_cls[n] == cls) obj_union_lds(s_par, v, n);
    }
  }
  __syncthreads();
  cls_out[id] = cls;
  cost[id] = is_free ? kNavUnreached : kNavBlocked;
  parent[id] = core ? slot * (uint32_t)kTileVoxels + obj_find_lds(s_par, v) : kObjNone;
}

// ---- seeds ----------------------------------------------------------------------------------------------------------------
// grid (nt * 2), 256 work-items: a wavefront is one z-layer of tile id >> 9.  comp: the voxels' provisional numbers (k_obj_reduce).
// write = 1: the room plane and the zero costs are made, write = 0: they are read.  Either way the tiles that hold a core voxel of
// a room enter list 0, once each.
__global__ void __launch_bounds__(256) k_room_seed(const uint32_t* __restrict__ comp, const uint32_t* __restrict__ final_of, int write, uint32_t* room,
                                                   uint32_t* cost, uint32_t* queued, uint32_t* __restrict__ list, uint32_t* count) {
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  uint32_t r;
  if (write) {
    const uint32_t c = comp[id];
    r = c == kObjNone ? kRoomNone : final_of[c];
    room[id] = r;
    if (r != kRoomNone) cost[id] = 0u;
  } else {
    r = cost[id] == 0u ? room[id] : kRoomNone;
  }
  const unsigned long long m = __ballot(r != kRoomNone);
  const uint32_t slot = id >> 9;
  const bool first = m && lane_id() == 0 && atomicExch(&queued[slot], 1u) == 0u;
  const uint32_t pos = wave_append(first, count);
  if (first) list[pos] = slot;
}

// ---- the room of every reached voxel ---------------------------------------------------------------------------------------------
// grid (n_tiles), 512 work-items; the layout of k_nav_relax.  F.cost is final and only read; room is the plane that decreases.
__global__ void __launch_bounds__(512) k_room_assign(TileTable T, NavField F, uint32_t* room, uint32_t* queued, uint32_t* lists, uint32_t* counts,
                                                     uint32_t round, NavCounters* __restrict__ C) {
  __shared__ uint32_t s_nb[27];
  __shared__ uint32_t s_tell[27];
  __shared__ uint32_t s_cost[1000];
  __shared__ uint32_t s_room[1000];
  __shared__ uint32_t s_any[3];
  const uint32_t v = threadIdx.x;
  const uint32_t n_active = counts[round % 3u];
  if (blockIdx.x == 0 && v == 0) {
    counts[(round + 2u) % 3u] = 0u;   // (read last in round - 1; round + 1 appends to it)
    if (n_active) {
      C->rounds += 1ull;              // (this work-item alone writes the two diagnostics)
      C->relaxations += (unsigned long long)n_active;
    }
  }
  if (blockIdx.x >= n_active) return;
  const uint32_t* list = lists + (size_t)(round & 1u) * F.n_tiles;
  uint32_t* list_next = lists + (size_t)((round + 1u) & 1u) * F.n_tiles;
  uint32_t* count_next = counts + (round + 1u) % 3u;
  const uint32_t slot = list[blockIdx.x];
  if (v < 27u) {
    int tx, ty, tz;
    unpack_tile(T.slot_keys[slot], tx, ty, tz);
    tx += (int)(v % 3u) - 1, ty += (int)((v / 3u) % 3u) - 1, tz += (int)(v / 9u) - 1;
    uint32_t s = kNavNoTile;
    if (tx >= -kTileBias && tx < kTileBias && ty >= -kTileBias && ty < kTileBias && tz >= -kTileBias && tz < kTileBias) {
      s = v == 13u ? slot : tile_lookup(T, pack_tile(tx, ty, tz));
      if (s >= F.n_tiles) s = kNavNoTile;
    }
    s_nb[v] = s;
    s_tell[v] = 0u;
  }
  if (v == 0) {
    s_any[0] = 0u;
    // as in k_nav_relax: from here on a neighbour that lowers a room we can see lists this tile again; one that found the flag
    // still set wrote before this exchange, and the fence below makes what it wrote visible to the loads of the halo
    atomicExch(&queued[slot], 0u);
  }
  __syncthreads();
  __threadfence();
  for (uint32_t c = v; c < 1000u; c += 512u) {
    const int hx = (int)(c % 10u) - 1, hy = (int)((c / 10u) % 10u) - 1, hz = (int)(c / 100u) - 1;
    const int t = (hx < 0 ? 0 : hx > 7 ? 2 : 1) + 3 * (hy < 0 ? 0 : hy > 7 ? 2 : 1) + 9 * (hz < 0 ? 0 : hz > 7 ? 2 : 1);
    const uint32_t ns = s_nb[t];
    const size_t at = (size_t)ns * kTileVoxels + obj_local(hx & 7, hy & 7, hz & 7);
    s_cost[c] = ns == kNavNoTile ? kNavBlocked : F.cost[at];
    s_room[c] = ns == kNavNoTile ? kRoomNone : nav_load(room + at);
  }
  __syncthreads();
  const int x = (int)(v & 7u), y = (int)((v >> 3) & 7u), z = (int)(v >> 6);
  const int cell = (x + 1) + 10 * (y + 1) + 100 * (z + 1);
  const uint32_t my_cost = s_cost[cell];
  const uint32_t before = s_room[cell];
  const bool takes = my_cost != 0u && my_cost <= kNavMaxCost;   // (a core of a room keeps its own; the rest has no path)
  uint32_t mine = before;
  // a sweep without a barrier inside: a neighbour's room of this sweep or of the last one, both are rooms with a shortest path
  // through that neighbour.  Sweep k ends with every voxel settled whose predecessors lie at most k steps inside the tile.
  for (int it = 0; it < kNavSweeps; ++it) {
    if (v == 0) s_any[(it + 1) % 3] = 0u;   // (read last in sweep it - 2, before the barrier of sweep it - 1)
    if (takes) {
      uint32_t m = mine;
#pragma unroll
      for (int o = 0; o < 27; ++o) {
        if (o == 13) continue;
        const int n = cell + (o % 3 - 1) + 10 * ((o / 3) % 3 - 1) + 100 * (o / 9 - 1);
        const uint32_t u = s_cost[n];
        if (u <= kNavMaxCost && u + nav_step_cost(o) == my_cost) {
          const uint32_t r = nav_lds_load(&s_room[n]);
          if (r < m) m = r;
        }
      }
      if (m < mine) {
        mine = m;
        nav_lds_store(&s_room[cell], m);
        s_any[it % 3] = 1u;
      }
    }
    __syncthreads();
    if (!s_any[it % 3]) break;   // (uniform)
  }
  const bool changed = mine != before;
  if (changed) nav_store(room + ((size_t)slot * kTileVoxels + v), mine);
  if (changed || (round == 0u && my_cost == 0u)) {   // (round 0 takes the seeded tiles: a core on the skin is news to the neighbours)
    const int sx = x == 0 ? -1 : x == 7 ? 1 : 0, sy = y == 0 ? -1 : y == 7 ? 1 : 0, sz = z == 0 ? -1 : z == 7 ? 1 : 0;
    for (int k = 1; k < 8; ++k) {
      if (((k & 1) && !sx) || ((k & 2) && !sy) || ((k & 4) && !sz)) continue;
      s_tell[(1 + ((k & 1) ? sx : 0)) + 3 * (1 + ((k & 2) ? sy : 0)) + 9 * (1 + ((k & 4) ? sz : 0))] = 1u;   // (every writer stores 1)
    }
  }
  __threadfence();   // the rooms are out before a neighbour can be told
  __syncthreads();
  if (v < 64u) {     // (the first wavefront, converged)
    bool first = false;
    uint32_t ns = kNavNoTile;
    if (v < 27u && v != 13u && s_tell[v]) {
      ns = s_nb[v];
      first = ns != kNavNoTile && atomicExch(&queued[ns], 1u) == 0u;
    }
    const uint32_t pos = wave_append(first, count_next);
    if (first) list_next[pos] = ns;
  }
}

// ---- reduce ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_room_acc_init(RoomAcc* __restrict__ acc, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  RoomAcc a;
  a.centre = ~0ull;
  for (int k = 0; k < 3; ++k) a.sum[k] = 0ull, a.bb_min[k] = 0x7fffffff, a.bb_max[k] = (int32_t)0x80000000u;
  a.n = a.largest_cost = a.clearance = a.n_links = a.n_objects = a.pad = 0u;
  acc[i] = a;
}

// grid (nt * 2), 256 work-items, a wavefront per z-layer of a tile as in k_obj_reduce
__global__ void __launch_bounds__(256) k_room_reduce(TileTable T, const EsdfRecord* __restrict__ store, const uint32_t* __restrict__ room,
                                                     const uint32_t* __restrict__ cost, RoomAcc* __restrict__ acc) {
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = lane_id();
  const uint32_t r = room[id];
  unsigned long long left = __ballot(r != kRoomNone);
  if (!left) return;   // (uniform)
  uint32_t cv = 0u, bits = 0u;
  if (r != kRoomNone) {
    cv = cost[id];
    if (cv == 0u) bits = __float_as_uint(store[id].distance);   // (a core voxel: its distance is finite and not negative)
  }
  int tx, ty, tz;
  unpack_tile(T.slot_keys[id >> 9], tx, ty, tz);
  const int lx = (int)(id & 7u), ly = (int)((id >> 3) & 7u), lz = (int)((id >> 6) & 7u);
  while (left) {
    const int leader = __ffsll((long long)left) - 1;
    const uint32_t c = __shfl(r, leader);
    const bool mine = r == c;
    const unsigned long long m = __ballot(mine);
    const uint32_t sums = obj_wave_add(mine ? (uint32_t)lx | ((uint32_t)ly << 10) | ((uint32_t)lz << 20) : 0u);
    const uint32_t occ = obj_wave_or(mine ? (1u << lx) | (1u << (8 + ly)) | (1u << (16 + lz)) : 0u);
    const uint32_t cmax = room_wave_max(mine ? cv : 0u);
    const uint32_t bmax = room_wave_max(mine ? bits : 0u);
    if ((int)lane == leader) {
      RoomAcc* A = acc + c;
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
      atomicMax(&A->largest_cost, cmax);
      if (bmax) atomicMax(&A->clearance, bmax);
    }
    left &= ~m;
  }
}

// grid (nt * 2), 256 work-items.  acc[].clearance is final (k_room_reduce has completed).
__global__ void __launch_bounds__(256) k_room_pick(TileTable T, const EsdfRecord* __restrict__ store, const uint32_t* __restrict__ room,
                                                   const uint32_t* __restrict__ cost, RoomAcc* __restrict__ acc) {
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  const uint32_t r = room[id];
  const bool hit = r != kRoomNone && cost[id] == 0u && __float_as_uint(store[id].distance) == acc[r].clearance;
  if (!hit) return;
  int gx, gy, gz;
  room_voxel_of(T, id, gx, gy, gz);
  atomicMin(&acc[r].centre, (unsigned long long)pack_coord3(gx, gy, gz));
}

// ---- contacts ---------------------------------------------------------------------------------------------------------------
// grid (nt), 512 work-items.  An incidence (v, q): v assigned to r, q != r the room of some 26-neighbour of v, counted once per q:
// at the first neighbour (in offset order) that shows it.  mode 0: *n_pairs += the incidences; mode 1: the pairs are appended.
__global__ void __launch_bounds__(512) k_room_contacts(TileTable T, uint32_t nt, const uint32_t* __restrict__ room, int mode, uint32_t* n_pairs,
                                                       uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  __shared__ uint32_t s_nb[27];
  __shared__ uint32_t s_room[1000];
  __shared__ uint32_t s_some;
  const uint32_t slot = blockIdx.x, v = threadIdx.x;
  if (v < 27u) {
    int tx, ty, tz;
    unpack_tile(T.slot_keys[slot], tx, ty, tz);
    tx += (int)(v % 3u) - 1, ty += (int)((v / 3u) % 3u) - 1, tz += (int)(v / 9u) - 1;
    uint32_t s = kNavNoTile;
    if (tx >= -kTileBias && tx < kTileBias && ty >= -kTileBias && ty < kTileBias && tz >= -kTileBias && tz < kTileBias) {
      s = v == 13u ? slot : tile_lookup(T, pack_tile(tx, ty, tz));
      if (s >= nt) s = kNavNoTile;
    }
    s_nb[v] = s;
  }
  if (v == 0) s_some = 0u;
  __syncthreads();
  for (uint32_t c = v; c < 1000u; c += 512u) {
    const int hx = (int)(c % 10u) - 1, hy = (int)((c / 10u) % 10u) - 1, hz = (int)(c / 100u) - 1;
    const int t = (hx < 0 ? 0 : hx > 7 ? 2 : 1) + 3 * (hy < 0 ? 0 : hy > 7 ? 2 : 1) + 9 * (hz < 0 ? 0 : hz > 7 ? 2 : 1);
    const uint32_t ns = s_nb[t];
    s_room[c] = ns == kNavNoTile ? kRoomNone : room[(size_t)ns * kTileVoxels + obj_local(hx & 7, hy & 7, hz & 7)];
  }
  __syncthreads();
  const int x = (int)(v & 7u), y = (int)((v >> 3) & 7u), z = (int)(v >> 6);
  const int cell = (x + 1) + 10 * (y + 1) + 100 * (z + 1);
  const uint32_t r = s_room[cell];
  bool some = false;
  if (r != kRoomNone) {
    for (int o = 0; o < 27; ++o) {
      const uint32_t q = s_room[cell + (o % 3 - 1) + 10 * ((o / 3) % 3 - 1) + 100 * (o / 9 - 1)];
      some = some || (q != kRoomNone && q != r);
    }
  }
  if (some) s_some = 1u;   // (every writer stores 1)
  __syncthreads();
  if (!s_some) return;     // (uniform: most tiles lie inside one room)
  uint32_t total = 0u;
  for (int o = 0; o < 27; ++o) {   // (uniform trip count: wave_append is called by whole wavefronts)
    bool emit = false;
    uint32_t q = kRoomNone;
    if (some) {
      q = s_room[cell + (o % 3 - 1) + 10 * ((o / 3) % 3 - 1) + 100 * (o / 9 - 1)];
      emit = q != kRoomNone && q != r;
      for (int p = 0; p < o && emit; ++p) emit = s_room[cell + (p % 3 - 1) + 10 * ((p / 3) % 3 - 1) + 100 * (p / 9 - 1)] != q;
    }
    if (mode == 0) {
      total += emit ? 1u : 0u;
    } else {
      const uint32_t pos = wave_append(emit, n_pairs);
      if (emit) {
        keys[pos] = r < q ? ((uint64_t)r << 32) | q : ((uint64_t)q << 32) | r;
        vals[pos] = slot * (uint32_t)kTileVoxels + v;
      }
    }
  }
  if (mode == 0) {
    total = obj_wave_add(total);
    if (lane_id() == 0 && total) atomicAdd(n_pairs, total);
  }
}

// One lane per sorted pair: the first of a run appends (key, position).
__global__ void __launch_bounds__(256) k_room_heads(const uint64_t* __restrict__ keys, uint32_t n, uint64_t* __restrict__ head_keys,
                                                    uint32_t* __restrict__ head_pos, uint32_t* n_links) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool head = i < n && (i == 0u || keys[i - 1u] != keys[i]);
  const uint32_t pos = wave_append(head, n_links);
  if (head) {
    head_keys[pos] = keys[i];
    head_pos[pos] = i;
  }
}

__global__ void __launch_bounds__(256) k_room_link_init(RoomLinkAcc* __restrict__ acc, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) acc[i] = RoomLinkAcc{~0ull, 0u, 0u};
}

// the link of sorted pair i: the last j with starts[j] <= i (starts ascend, starts[0] == 0)
__device__ __forceinline__ uint32_t room_link_of(const uint32_t* __restrict__ starts, uint32_t n_links, uint32_t i) {
  uint32_t lo = 0u, hi = n_links;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (starts[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One lane per sorted pair, pass one: the largest distance bits of the link's contacts.
__global__ void __launch_bounds__(256) k_room_link_max(const EsdfRecord* __restrict__ store, const uint32_t* __restrict__ vals, uint32_t n,
                                                       const uint32_t* __restrict__ starts, uint32_t n_links, RoomLinkAcc* __restrict__ acc) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  atomicMax(&acc[room_link_of(starts, n_links, i)].clearance, __float_as_uint(store[vals[i]].distance));
}

// ... pass two: the smallest voxel among those at the largest bits
__global__ void __launch_bounds__(256) k_room_link_pick(TileTable T, const EsdfRecord* __restrict__ store, const uint32_t* __restrict__ vals, uint32_t n,
                                                        const uint32_t* __restrict__ starts, uint32_t n_links, RoomLinkAcc* __restrict__ acc) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  RoomLinkAcc* A = acc + room_link_of(starts, n_links, i);
  const uint32_t id = vals[i];
  if (__float_as_uint(store[id].distance) != A->clearance) return;
  int gx, gy, gz;
  room_voxel_of(T, id, gx, gy, gz);
  atomicMin(&A->door, (unsigned long long)pack_coord3(gx, gy, gz));
}

// One lane per link.  door_room is read from the plane, at the door voxel through the tile table.
__global__ void __launch_bounds__(256) k_room_links(TileTable T, uint32_t nt, const uint32_t* __restrict__ room, const uint64_t* __restrict__ head_keys,
                                                    const uint32_t* __restrict__ starts, uint32_t n_links, uint32_t n_pairs,
                                                    const RoomLinkAcc* __restrict__ lacc, RoomAcc* __restrict__ acc, ks_room_link* __restrict__ out) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n_links) return;
  const uint64_t key = head_keys[j];
  ks_room_link L;
  L.room_a = (uint32_t)(key >> 32);
  L.room_b = (uint32_t)key;
  L.n_contacts = (j + 1u < n_links ? starts[j + 1u] : n_pairs) - starts[j];
  L.clearance_bits = lacc[j].clearance;
  unpack_coord3((uint64_t)lacc[j].door, L.door_voxel[0], L.door_voxel[1], L.door_voxel[2]);
  const uint32_t slot = tile_lookup(T, pack_tile(L.door_voxel[0] >> 3, L.door_voxel[1] >> 3, L.door_voxel[2] >> 3));
  L.door_room = slot < nt ? room[(size_t)slot * kTileVoxels + obj_local(L.door_voxel[0] & 7, L.door_voxel[1] & 7, L.door_voxel[2] & 7)] : kRoomNone;
  out[j] = L;
  atomicAdd(&acc[L.room_a].n_links, 1u);
  atomicAdd(&acc[L.room_b].n_links, 1u);
}

// ---- the join with the objects ---------------------------------------------------------------------------------------------
// grid ceil(n / 256), 256 work-items; n = 512 * the slots both id stores cover
__global__ void __launch_bounds__(256) k_room_obj_min(const uint32_t* __restrict__ obj_ids, uint32_t n_objects, const uint32_t* __restrict__ room,
                                                      const uint32_t* __restrict__ cost, size_t n, unsigned long long* __restrict__ best) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = obj_ids[i];
  if (o >= n_objects) return;   // (kObjNone included)
  const uint32_t r = room[i];
  if (r != kRoomNone) atomicMin(&best[o], ((unsigned long long)cost[i] << 32) | r);
}

__global__ void __launch_bounds__(256) k_room_obj_join(const unsigned long long* __restrict__ best, uint32_t n_objects, uint32_t* __restrict__ room_of,
                                                       RoomAcc* __restrict__ acc, RoomCounters* __restrict__ C) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool joined = false;
  if (i < n_objects) {
    const unsigned long long b = best[i];
    joined = b != ~0ull;
    room_of[i] = joined ? (uint32_t)b : kRoomNone;
    if (joined) atomicAdd(&acc[(uint32_t)b].n_objects, 1u);
  }
  const unsigned long long m = __ballot(joined);
  if (lane_id() == 0 && m) atomicAdd(&C->objects_joined, (uint32_t)__popcll(m));
}

// ---- records ----------------------------------------------------------------------------------------------------------------
// One lane per room.  cores: k_obj_records' records of the rooms' core components, in room order.
__global__ void __launch_bounds__(256) k_room_records(const ks_object* __restrict__ cores, const RoomAcc* __restrict__ acc, uint32_t n_rooms,
                                                      ks_room* __restrict__ out, RoomCounters* __restrict__ C) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t nv = 0u, big_cost = 0u;
  if (i < n_rooms) {
    const ks_object o = cores[i];
    const RoomAcc a = acc[i];
    ks_room r;
    for (int k = 0; k < 3; ++k) r.first_voxel[k] = o.first_voxel[k], r.bb_min[k] = a.bb_min[k], r.bb_max[k] = a.bb_max[k], r.sum[k] = (int64_t)a.sum[k];
    r.n_core_voxels = o.n_voxels;
    r.n_voxels = a.n;
    r.largest_cost = a.largest_cost;
    r.clearance_bits = a.clearance;
    unpack_coord3((uint64_t)a.centre, r.centre_voxel[0], r.centre_voxel[1], r.centre_voxel[2]);
    r.n_links = a.n_links;
    r.n_objects = a.n_objects;
    out[i] = r;
    nv = a.n;
    big_cost = a.largest_cost;
  }
  const unsigned long long m = __ballot(nv != 0u);
  const uint32_t total = obj_wave_add(nv);
  const uint32_t big = room_wave_max(nv), bc = room_wave_max(big_cost);
  if (lane_id() == 0 && m) {
    atomicAdd(&C->assigned, (unsigned long long)total);
    atomicMax(&C->largest_room, big);
    atomicMax(&C->largest_cost, bc);
  }
}

}  // namespace ksk
