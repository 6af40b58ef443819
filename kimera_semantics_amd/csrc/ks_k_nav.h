// ks_k_nav.h — the navigation field over the stored ESDF: per voxel of the store's tiles the integer cost-to-go to the nearest of
// a set of goals through the voxels a sphere of a given radius may occupy (26-connected, steps of 10 / 14 / 17), and the paths
// that descend it.  The contract (traversable, graph, goals, field, cap, the walk of a path) is DESIGN.md, section "Navigation
// field"; tests/nav_model.py restates it in NumPy and the kernels are compared with it byte for byte.  The ESDF store is only read.
//
// The field is the unique fixed point of  f(v) = min(f(v), min over neighbours u of f(u) + w(u, v))  from f(goal) = 0: every value
// ever stored is the cost of a real path and values only decrease, so whatever a tile reads of its neighbours — before or after
// they wrote — the iteration ends at the shortest-path costs.  One word per voxel, `field[slot * 512 + local]`.
//
//   k_nav_init    a lane per voxel of the store's tiles: kNavBlocked or kNavUnreached from the ESDF record
//   k_nav_seed    a lane per goal: its voxel through the tile table; a traversable one gets cost 0 and its tile enters list 0
//   k_nav_relax   one workgroup per ACTIVE tile (the grid covers every tile; workgroups beyond the list's count return at once):
//                 the slots of the 26 neighbour tiles and the 10 x 10 x 10 halo of costs into LDS, then every own traversable
//                 voxel takes the minimum over its 26 neighbours until nothing changes (at most 513 sweeps).  The own tile's
//                 changed costs are written by this workgroup alone; a changed voxel on the tile's skin (in round 0 also a goal
//                 voxel there) puts the up to 7 neighbour tiles that see it on the NEXT list.  `queued[tile]` is 1 while the tile waits on a list: taken with
//                 atomicExch, so a tile is listed once; the tile itself clears it BEFORE it reads its halo, so a neighbour that
//                 finds it set knows the tile has yet to read what the neighbour just wrote.
//                 Round r reads counts[r % 3], appends to counts[(r + 1) % 3] and clears counts[(r + 2) % 3] for round r + 1.
//   k_nav_count   voxels reached and the largest cost (integer add / max, one atomic per wavefront)
//   k_nav_paths   a lane per start: steepest descent in a for loop of at most max_waypoints iterations; the lane's TileMemo
//                 carries from step to step
// The block download and the point query of the field are those of every one-word-per-voxel store whose "nothing here" is
// all-ones (k_obj_download, k_obj_query in ks_k_objects.h): kNavBlocked == kObjNone.
// No floating-point atomics, no atomics on costs (the seeds store 0 with a plain store: every writer stores the same value).
#pragma once
#include "ks_k_esdf.h"
#include "ks_k_objects.h"
#include "ks_k_render.h"

namespace ksk {

constexpr uint32_t kNavBlocked = KS_NAV_BLOCKED, kNavUnreached = KS_NAV_UNREACHED, kNavMaxCost = KS_NAV_MAX_COST;
constexpr uint32_t kNavNoTile = 0xffffffffu;
constexpr int kNavSweeps = 513;   // 512 nodes against a fixed halo: a sweep settles at least one more voxel, the last finds no change
static_assert(kNavBlocked == kObjNone, "the field is read by the id store's download and query kernels");
static_assert((uint64_t)kNavMaxCost + KS_NAV_COST_CORNER < kNavUnreached, "a reached cost plus a step never wraps or meets a marker");

struct NavCounters {   // 64 B
  unsigned long long traversable, reached, largest, goals_used, goals_blocked, rounds, relaxations, pad;
};

struct NavField {
  uint32_t* cost;      // [n_tiles][512]
  uint32_t n_tiles;    // the tiles of the ESDF store the field was made from: a slot at or above reads as kNavBlocked
};

struct NavPaths {
  const float* starts;   // [n][3]
  size_t n;
  uint32_t max_waypoints;
  float voxel_size, voxel_size_inv;
  uint8_t* status;       // [n]                      any of the four may be nullptr
  uint32_t* cost;        // [n]
  uint32_t* n_waypoints; // [n]
  float* waypoints;      // [n][max_waypoints][3]
  unsigned long long* counters;   // reached | unreachable | blocked | truncated | waypoints
};

// the step cost of offset o = dx + 1 + 3 * (dy + 1) + 9 * (dz + 1)
__host__ __device__ constexpr uint32_t nav_step_cost(int o) {
  const int k = (o % 3 != 1) + ((o / 3) % 3 != 1) + (o / 9 != 1);
  return k == 1 ? KS_NAV_COST_FACE : k == 2 ? KS_NAV_COST_EDGE : KS_NAV_COST_CORNER;
}

// costs travel between workgroups while both run: single-copy atomic 32-bit accesses at agent scope (plain loads and stores
// that the caches of another compute unit cannot hold back)
__device__ __forceinline__ uint32_t nav_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void nav_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// ... and between the work-items of a workgroup through LDS, inside a sweep without a barrier
__device__ __forceinline__ uint32_t nav_lds_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void nav_lds_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// grid ceil(n / 256), 256 work-items; n = n_tiles * 512
__global__ void __launch_bounds__(256) k_nav_init(const EsdfRecord* __restrict__ store, size_t n, float radius, uint32_t* __restrict__ cost,
                                                  NavCounters* __restrict__ C) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  bool traversable = false;
  if (i < n) {
    const EsdfRecord r = store[i];
    traversable = (r.tail & 1u) && r.distance >= radius;   // (a NaN distance is not traversable)
    cost[i] = traversable ? kNavUnreached : kNavBlocked;
  }
  const unsigned long long m = __ballot(traversable);
  if (lane_id() == 0 && m) atomicAdd(&C->traversable, (unsigned long long)__popcll(m));
}

// grid ceil(n_goals / 256), 256 work-items.  The voxel of a goal is the one k_esdf_query takes for the point.
__global__ void __launch_bounds__(256) k_nav_seed(TileTable T, NavField F, const float* __restrict__ goals, uint32_t n_goals, float voxel_size_inv,
                                                  uint32_t* queued, uint32_t* __restrict__ list, uint32_t* count, NavCounters* __restrict__ C) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool live = i < n_goals;
  bool used = false;
  uint32_t slot = kNavNoTile;
  if (live) {
    const float gx = grid_coord(goals[3 * i], voxel_size_inv), gy = grid_coord(goals[3 * i + 1], voxel_size_inv),
                gz = grid_coord(goals[3 * i + 2], voxel_size_inv);
    const float lim = (float)(kCoordBias - 1);
    if (fabsf(gx) < lim && fabsf(gy) < lim && fabsf(gz) < lim) {   // (false for a coordinate that is not finite)
      const int vx = (int)gx, vy = (int)gy, vz = (int)gz;
      slot = tile_lookup(T, pack_tile(vx >> 3, vy >> 3, vz >> 3));
      if (slot < F.n_tiles) {
        uint32_t* at = F.cost + ((size_t)slot * kTileVoxels + esdf_local(vx, vy, vz));
        if (nav_load(at) != kNavBlocked) {
          nav_store(at, 0u);
          used = true;
        }
      }
    }
  }
  const unsigned long long m_used = __ballot(used), m_blocked = __ballot(live && !used);
  if (lane_id() == 0) {
    if (m_used) atomicAdd(&C->goals_used, (unsigned long long)__popcll(m_used));
    if (m_blocked) atomicAdd(&C->goals_blocked, (unsigned long long)__popcll(m_blocked));
  }
  const bool first = used && atomicExch(&queued[slot], 1u) == 0u;
  const uint32_t pos = wave_append(first, count);
  if (first) list[pos] = slot;
}

// grid (n_tiles), 512 work-items.  s_nb[o]: the slot of the tile at offset o (o = dx + 1 + 3 * (dy + 1) + 9 * (dz + 1), 13 = this
// tile), kNavNoTile where the field has none.  s_cost: the halo, cell (hx + 1) + 10 * (hy + 1) + 100 * (hz + 1) for the local
// coordinates -1..8.  lists: [2][n_tiles], round r reads lists[r & 1].
__global__ void __launch_bounds__(512) k_nav_relax(TileTable T, NavField F, uint32_t* queued, uint32_t* lists, uint32_t* counts, uint32_t round,
                                                   uint32_t max_cost, NavCounters* __restrict__ C) {
  __shared__ uint32_t s_nb[27];
  __shared__ uint32_t s_tell[27];
  __shared__ uint32_t s_cost[1000];
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
    // from here on a neighbour that changes a cost we can see lists this tile again; one that found the flag still set wrote
    // before this exchange, and the fence below makes what it wrote visible to the loads of the halo
    atomicExch(&queued[slot], 0u);
  }
  __syncthreads();
  __threadfence();
  for (uint32_t c = v; c < 1000u; c += 512u) {
    const int hx = (int)(c % 10u) - 1, hy = (int)((c / 10u) % 10u) - 1, hz = (int)(c / 100u) - 1;
    const int t = (hx < 0 ? 0 : hx > 7 ? 2 : 1) + 3 * (hy < 0 ? 0 : hy > 7 ? 2 : 1) + 9 * (hz < 0 ? 0 : hz > 7 ? 2 : 1);
    const uint32_t ns = s_nb[t];
    s_cost[c] = ns == kNavNoTile ? kNavBlocked : nav_load(F.cost + ((size_t)ns * kTileVoxels + obj_local(hx & 7, hy & 7, hz & 7)));
  }
  __syncthreads();
  const int x = (int)(v & 7u), y = (int)((v >> 3) & 7u), z = (int)(v >> 6);
  const int cell = (x + 1) + 10 * (y + 1) + 100 * (z + 1);
  const uint32_t before = s_cost[cell];
  const bool traversable = before != kNavBlocked;
  uint32_t mine = before;
  // a sweep without a barrier inside: a work-item may read a neighbour's cost of this sweep or of the last one, both are costs
  // of real paths.  Sweep k ends with every voxel settled whose shortest path (against this halo) has at most k steps in the tile.
  for (int it = 0; it < kNavSweeps; ++it) {
    if (v == 0) s_any[(it + 1) % 3] = 0u;   // (read last in sweep it - 2, before the barrier of sweep it - 1)
    if (traversable) {
      uint32_t m = mine;
#pragma unroll
      for (int o = 0; o < 27; ++o) {
        if (o == 13) continue;
        const uint32_t u = nav_lds_load(&s_cost[cell + (o % 3 - 1) + 10 * ((o / 3) % 3 - 1) + 100 * (o / 9 - 1)]);
        const uint32_t via = u + nav_step_cost(o);
        if (u <= kNavMaxCost && via < m) m = via;
      }
      if (m < mine && m <= max_cost) {   // (a result above the cap is dropped)
        mine = m;
        nav_lds_store(&s_cost[cell], m);
        s_any[it % 3] = 1u;
      }
    }
    __syncthreads();
    if (!s_any[it % 3]) break;   // (uniform)
  }
  const bool changed = mine != before;
  if (changed) nav_store(F.cost + ((size_t)slot * kTileVoxels + v), mine);
  if (changed || (round == 0u && mine == 0u)) {   // (round 0 takes the seeded tiles: a goal voxel is news to the neighbours too)
    // the neighbour tiles whose halo holds this voxel: every non-empty choice of the axes on which it lies on the skin
    const int sx = x == 0 ? -1 : x == 7 ? 1 : 0, sy = y == 0 ? -1 : y == 7 ? 1 : 0, sz = z == 0 ? -1 : z == 7 ? 1 : 0;
    for (int k = 1; k < 8; ++k) {
      if (((k & 1) && !sx) || ((k & 2) && !sy) || ((k & 4) && !sz)) continue;
      s_tell[(1 + ((k & 1) ? sx : 0)) + 3 * (1 + ((k & 2) ? sy : 0)) + 9 * (1 + ((k & 4) ? sz : 0))] = 1u;   // (every writer stores 1)
    }
  }
  __threadfence();   // the costs are out before a neighbour can be told
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

// grid ceil(n / 256), 256 work-items
__global__ void __launch_bounds__(256) k_nav_count(const uint32_t* __restrict__ cost, size_t n, NavCounters* __restrict__ C) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t c = i < n ? cost[i] : kNavBlocked;
  const bool reached = c <= kNavMaxCost;
  const unsigned long long m = __ballot(reached);
  uint32_t big = reached ? c : 0u;
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t u = __shfl_xor(big, o);
    big = u > big ? u : big;
  }
  if (lane_id() == 0 && m) {
    atomicAdd(&C->reached, (unsigned long long)__popcll(m));
    atomicMax(&C->largest, (unsigned long long)big);
  }
}

// the cost of voxel (x, y, z): kNavBlocked outside the tile range and where the field has no tile
__device__ __forceinline__ uint32_t nav_read(const TileTable& T, const NavField& F, TileMemo& M, int x, int y, int z) {
  const int tx = x >> 3, ty = y >> 3, tz = z >> 3;
  if (!(tx >= -kTileBias && tx < kTileBias && ty >= -kTileBias && ty < kTileBias && tz >= -kTileBias && tz < kTileBias)) return kNavBlocked;
  const uint32_t slot = render_slot(T, M, tx, ty, tz);
  return slot < F.n_tiles ? F.cost[(size_t)slot * kTileVoxels + esdf_local(x, y, z)] : kNavBlocked;
}

// grid ceil(n / 256), 256 work-items
__global__ void __launch_bounds__(256) k_nav_paths(TileTable T, NavField F, NavPaths P) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  const bool live = i < P.n;
  uint32_t status = KS_NAV_PATH_INVALID, written = 0u;
  if (live) {
    const float gx = grid_coord(P.starts[3 * i], P.voxel_size_inv), gy = grid_coord(P.starts[3 * i + 1], P.voxel_size_inv),
                gz = grid_coord(P.starts[3 * i + 2], P.voxel_size_inv);
    const float lim = (float)(kCoordBias - 1);
    TileMemo M;
    int vx = 0, vy = 0, vz = 0;
    uint32_t cur = kNavBlocked;
    if (fabsf(gx) < lim && fabsf(gy) < lim && fabsf(gz) < lim) {
      vx = (int)gx, vy = (int)gy, vz = (int)gz;
      cur = nav_read(T, F, M, vx, vy, vz);
    }
    if (P.cost) P.cost[i] = cur;
    if (cur == kNavBlocked) {
      status = KS_NAV_PATH_BLOCKED;
    } else if (cur > kNavMaxCost) {
      status = KS_NAV_PATH_UNREACHABLE;
    } else {
      status = KS_NAV_PATH_TRUNCATED;   // what a walk is that the loop's bound ends
      float* wp = P.waypoints ? P.waypoints + i * (size_t)P.max_waypoints * 3u : nullptr;
      for (uint32_t it = 0; it < P.max_waypoints; ++it) {
        if (wp) {
          wp[3 * (size_t)it] = ((float)vx + 0.5f) * P.voxel_size;
          wp[3 * (size_t)it + 1] = ((float)vy + 0.5f) * P.voxel_size;
          wp[3 * (size_t)it + 2] = ((float)vz + 0.5f) * P.voxel_size;
        }
        written = it + 1u;
        if (cur == 0u) {
          status = KS_NAV_PATH_REACHED;
          break;
        }
        int next = -1;
        uint32_t next_cost = 0u;
        for (int o = 0; o < 27 && next < 0; ++o) {
          if (o == 13) continue;
          const uint32_t u = nav_read(T, F, M, vx + o % 3 - 1, vy + (o / 3) % 3 - 1, vz + o / 9 - 1);
          if (u <= kNavMaxCost && u + nav_step_cost(o) == cur) next = o, next_cost = u;
        }
        if (next < 0) {   // (not on a field this library made)
          status = KS_NAV_PATH_INVALID;
          break;
        }
        vx += next % 3 - 1, vy += (next / 3) % 3 - 1, vz += next / 9 - 1;
        cur = next_cost;
      }
    }
    if (P.status) P.status[i] = (uint8_t)status;
    if (P.n_waypoints) P.n_waypoints[i] = written;
  }
  // the wavefront is converged again: its five sums, one atomic each
  const unsigned long long m_reached = __ballot(live && status == KS_NAV_PATH_REACHED), m_unreach = __ballot(live && status == KS_NAV_PATH_UNREACHABLE);
  const unsigned long long m_blocked = __ballot(live && status == KS_NAV_PATH_BLOCKED), m_trunc = __ballot(live && status == KS_NAV_PATH_TRUNCATED);
  const uint32_t total = obj_wave_add(written);
  if (lane_id() == 0) {
    if (m_reached) atomicAdd(&P.counters[0], (unsigned long long)__popcll(m_reached));
    if (m_unreach) atomicAdd(&P.counters[1], (unsigned long long)__popcll(m_unreach));
    if (m_blocked) atomicAdd(&P.counters[2], (unsigned long long)__popcll(m_blocked));
    if (m_trunc) atomicAdd(&P.counters[3], (unsigned long long)__popcll(m_trunc));
    if (total) atomicAdd(&P.counters[4], (unsigned long long)total);
  }
}

}  // namespace ksk
