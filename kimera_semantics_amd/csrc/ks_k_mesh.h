// ks_k_mesh.h — semantic mesh extraction from the device-resident map: marching cubes over the 8^3 tiles of the pool,
// reading the 128-byte voxel records in place.  The contract (cube ownership, corner / edge numbering, vertex rule,
// normals, attributes, order) is DESIGN.md, section "Semantic mesh"; tests/mesh_model.py restates it in NumPy and the
// kernels are compared with it bit for bit.
//
//   k_mesh_tiles<false>  counting pass: one workgroup per (block to re-mesh, tile of the block), one lane per cube; the 9^3
//                        halo of (distance, weight) is staged in LDS once; per cube the number of triangles that survive
//                        the degenerate test -> cube_cnt (block-linear cube order)
//   k_mesh_scan          one workgroup per block: exclusive scan of its cubes' counts, the block's total
//   k_mesh_dir           one workgroup: exclusive scan of the vertex counts of ALL blocks of the new directory (re-meshed
//                        ones from the totals, kept ones from the old directory) -> first vertex of every block
//   k_mesh_tiles<true>   emitting pass: the same walk with colour and label staged too; every triangle is written at the
//                        position the scans gave it — no atomic decides a position, two runs give the same bytes
//   k_mesh_copy          segments of the blocks that were not re-meshed move from the old arena to the new one
#pragma once
#include "ks_types.h"

namespace ksk {

// 256 x 16 triangle table: the ONE copy is the data file (its header documents the numbering).
alignas(16) static __device__ const int8_t kMcTriTable[256 * 16] = {
#include "ks_mc_tri_table.inc"
};

struct MeshArena {   // the mesh on the device: three vertices per triangle, segments of blocks back to back
  float* xyz;        // [n_vertices][3]
  float* nrm;        // [n_vertices][3]  the triangle's normal, repeated for its three vertices
  uint32_t* rgba;    // [n_vertices]     dword 2 of the record of the voxel whose cell contains the vertex
  uint8_t* label;    // [n_vertices]     its arg-max label (0 for a voxel the semantic side never updated, as ks_download_blocks shows it)
};

struct MeshWork {
  const int32_t* rblocks;   // [n_r][3] host-layout block indices to re-mesh, ascending (x, y, z)
  uint8_t* cube_cnt;        // [n_r][vps^3] triangles per cube (block-linear order x + vps * (y + vps * z))
  uint32_t* cube_off;       // [n_r][vps^3] exclusive scan of cube_cnt inside the block
  uint32_t* block_tri;      // [n_r] triangles of the block
  uint32_t* rb_first;       // [n_r] first vertex of the block's new segment
  unsigned long long* degenerate;   // triangles dropped by the counting pass (a statistic, decides no position)
  float voxel_size;
  float min_weight;
  int vps_shift;            // log2(vps / 8)
};

constexpr int kHalo = 9;
constexpr int kHaloVoxels = kHalo * kHalo * kHalo;   // 729

struct McVertex {
  float x, y, z;
  uint32_t owner;   // LDS index of the voxel whose cell contains the vertex
};

// Vertex on edge e of the cube whose lowest corner sits at halo index i0 / voxel (gx, gy, gz): always evaluated from the
// lower-numbered corner a, t = da / (da - db), p = pa + t * (pb - pa) per component (voxel centres).  Corner and halo index
// follow from e by arithmetic (no table in registers, nothing a lane-dependent index could push to scratch memory).
template <int STRIDE>
__device__ __forceinline__ McVertex mc_vertex(const uint32_t* halo, int e, uint32_t i0, int gx, int gy, int gz, float vs) {
  const int axis = e >> 2, j = e & 3;
  const int a = axis == 0 ? 2 * j : (axis == 1 ? (j & 1) + 4 * (j >> 1) : j);
  const int ax = a & 1, ay = (a >> 1) & 1, az = a >> 2;
  const int bx = ax + (axis == 0), by = ay + (axis == 1), bz = az + (axis == 2);
  const uint32_t ia = i0 + (uint32_t)(ax + kHalo * (ay + kHalo * az));
  const uint32_t ib = i0 + (uint32_t)(bx + kHalo * (by + kHalo * bz));
  const float da = __uint_as_float(halo[ia * STRIDE]), db = __uint_as_float(halo[ib * STRIDE]);
  const float pax = ((float)(gx + ax) + 0.5f) * vs, pay = ((float)(gy + ay) + 0.5f) * vs, paz = ((float)(gz + az) + 0.5f) * vs;
  const float pbx = ((float)(gx + bx) + 0.5f) * vs, pby = ((float)(gy + by) + 0.5f) * vs, pbz = ((float)(gz + bz) + 0.5f) * vs;
  const float t = da / (da - db);
  McVertex v;
  v.x = pax + t * (pbx - pax);
  v.y = pay + t * (pby - pay);
  v.z = paz + t * (pbz - paz);
  v.owner = t < 0.5f ? ia : ib;
  return v;
}

template <bool EMIT>
__global__ void __launch_bounds__(512) k_mesh_tiles(TileTable T, Pool P, MeshWork W, MeshArena A) {
  constexpr int STRIDE = EMIT ? 4 : 2;   // dwords staged per voxel: distance, weight (, colour, label)
  __shared__ uint32_t s_halo[kHaloVoxels * STRIDE];
  __shared__ int8_t s_tri[256 * 16];
  __shared__ uint32_t s_slot[8];
  const int tpb_shift = W.vps_shift, tpb = 1 << tpb_shift;   // tiles per block edge
  const uint32_t rb = blockIdx.x >> (3 * tpb_shift);
  const uint32_t tin = blockIdx.x & ((1u << (3 * tpb_shift)) - 1u);
  const int tix = (int)(tin & (uint32_t)(tpb - 1)), tiy = (int)((tin >> tpb_shift) & (uint32_t)(tpb - 1)), tiz = (int)(tin >> (2 * tpb_shift));
  const int tx = W.rblocks[3 * rb] * tpb + tix, ty = W.rblocks[3 * rb + 1] * tpb + tiy, tz = W.rblocks[3 * rb + 2] * tpb + tiz;
  if (threadIdx.x < 8) {
    const int dx = (int)(threadIdx.x & 1u), dy = (int)((threadIdx.x >> 1) & 1u), dz = (int)(threadIdx.x >> 2);
    const int nx = tx + dx, ny = ty + dy, nz = tz + dz;
    uint32_t slot = 0xffffffffu;
    if (nx < kTileBias && ny < kTileBias && nz < kTileBias) slot = tile_lookup(T, pack_tile(nx, ny, nz));
    s_slot[threadIdx.x] = slot < T.max_tiles ? slot : 0xffffffffu;
  }
  for (uint32_t i = threadIdx.x; i < 256u * 16u / 4u; i += 512u) ((uint32_t*)s_tri)[i] = ((const uint32_t*)kMcTriTable)[i];
  __syncthreads();
  // a tile that is not resident holds default voxels (weight 0): none of its cubes is meshed (cube_cnt is zeroed beforehand)
  if (s_slot[0] == 0xffffffffu) return;
  for (uint32_t i = threadIdx.x; i < (uint32_t)kHaloVoxels; i += 512u) {
    const uint32_t hx = i % kHalo, hy = (i / kHalo) % kHalo, hz = i / (kHalo * kHalo);
    const uint32_t slot = s_slot[(hx >> 3) + 2u * (hy >> 3) + 4u * (hz >> 3)];
    const uint32_t local = (hx & 7u) + 8u * ((hy & 7u) + 8u * (hz & 7u));
    if (EMIT) {
      uint4 q = make_uint4(0u, 0u, 0u, 255u);
      if (slot != 0xffffffffu) q = P.vox[((size_t)slot * kTileVoxels + local) * 8];
      s_halo[i * STRIDE] = q.x;
      s_halo[i * STRIDE + 1] = q.y;
      s_halo[i * STRIDE + 2] = q.z;
      s_halo[i * STRIDE + 3] = q.w;
    } else {
      uint2 q = make_uint2(0u, 0u);
      if (slot != 0xffffffffu) q = *(const uint2*)(P.vox + ((size_t)slot * kTileVoxels + local) * 8);
      s_halo[i * STRIDE] = q.x;
      s_halo[i * STRIDE + 1] = q.y;
    }
  }
  __syncthreads();
  const int x = (int)(threadIdx.x & 7u), y = (int)((threadIdx.x >> 3) & 7u), z = (int)(threadIdx.x >> 6);
  const uint32_t i0 = (uint32_t)(x + kHalo * (y + kHalo * z));
  bool all = true;
  uint32_t cs = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t at = (i0 + (uint32_t)((i & 1) + kHalo * (((i >> 1) & 1) + kHalo * (i >> 2)))) * STRIDE;
    const float d = __uint_as_float(s_halo[at]), w = __uint_as_float(s_halo[at + 1]);
    all = all && (w >= W.min_weight);
    if (d < 0.0f) cs |= 1u << i;
  }
  const int vps = 8 << tpb_shift;
  const uint32_t linear = (uint32_t)((tix * 8 + x) + vps * ((tiy * 8 + y) + vps * (tiz * 8 + z)));
  const size_t cube = ((size_t)rb << (9 + 3 * tpb_shift)) + linear;
  const int gx = tx * 8 + x, gy = ty * 8 + y, gz = tz * 8 + z;
  uint32_t n_tri = 0, n_deg = 0;
  size_t vout = 0;
  if (EMIT) vout = (size_t)W.rb_first[rb] + 3u * (size_t)W.cube_off[cube];
  if (all) {
    const int8_t* row = s_tri + cs * 16u;
    for (int k = 0; k < 15; k += 3) {
      const int e0 = row[k];
      if (e0 < 0) break;
      const McVertex v0 = mc_vertex<STRIDE>(s_halo, e0, i0, gx, gy, gz, W.voxel_size);
      const McVertex v1 = mc_vertex<STRIDE>(s_halo, row[k + 1], i0, gx, gy, gz, W.voxel_size);
      const McVertex v2 = mc_vertex<STRIDE>(s_halo, row[k + 2], i0, gx, gy, gz, W.voxel_size);
      const float ux = v1.x - v0.x, uy = v1.y - v0.y, uz = v1.z - v0.z;
      const float wx = v2.x - v0.x, wy = v2.y - v0.y, wz = v2.z - v0.z;
      const float cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
      const float len = sqrtf(cx * cx + cy * cy + cz * cz);
      if (len == 0.0f) {   // dropped, and counted
        ++n_deg;
        continue;
      }
      if (EMIT) {
        const float nx = cx / len, ny = cy / len, nz = cz / len;
        const McVertex vv[3] = {v0, v1, v2};
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          const size_t o = vout + (size_t)m;
          A.xyz[3 * o] = vv[m].x;
          A.xyz[3 * o + 1] = vv[m].y;
          A.xyz[3 * o + 2] = vv[m].z;
          A.nrm[3 * o] = nx;
          A.nrm[3 * o + 1] = ny;
          A.nrm[3 * o + 2] = nz;
          A.rgba[o] = s_halo[vv[m].owner * STRIDE + (STRIDE - 2)];
          const uint32_t lab = s_halo[vv[m].owner * STRIDE + (STRIDE - 1)];
          A.label[o] = (uint8_t)(lab == 255u ? 0u : lab);
        }
        vout += 3;
      }
      ++n_tri;
    }
  }
  if (!EMIT) {
    W.cube_cnt[cube] = (uint8_t)n_tri;
    if (n_deg) atomicAdd(W.degenerate, (unsigned long long)n_deg);
  }
}

// one workgroup per re-meshed block: exclusive scan of the triangle counts of its vps^3 cubes, total in block_tri
__global__ void __launch_bounds__(1024) k_mesh_scan(MeshWork W) {
  __shared__ uint32_t s_wave[16];
  __shared__ uint32_t s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  const uint32_t nv = 512u << (3 * W.vps_shift);
  const uint8_t* cnt = W.cube_cnt + (size_t)blockIdx.x * nv;
  uint32_t* off = W.cube_off + (size_t)blockIdx.x * nv;
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  for (uint32_t base = 0; base < nv; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nv ? (uint32_t)cnt[i] : 0u;
    uint32_t xs = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t ys = __shfl_up(xs, o);
      if (lane >= (uint32_t)o) xs += ys;
    }
    if (lane == 63) s_wave[wave] = xs;
    __syncthreads();
    uint32_t add = s_carry;
    for (uint32_t w = 0; w < wave; ++w) add += s_wave[w];
    if (i < nv) off[i] = add + xs - v;
    __syncthreads();
    if (threadIdx.x == 1023) s_carry = add + xs;
    __syncthreads();
  }
  if (threadIdx.x == 0) W.block_tri[blockIdx.x] = s_carry;
}

// The new block directory.  dir_in[i] = {r, n}: r = number of the block among the re-meshed ones (its vertex count comes
// from block_tri) or 0xffffffff for a block whose segment is kept (n = its vertex count).  dir_out[i] = first vertex of
// block i, dir_out[nb] = vertices in all; dir_n[i] = vertex count of block i.
__global__ void __launch_bounds__(1024) k_mesh_dir(MeshWork W, const uint2* __restrict__ dir_in, uint32_t nb,
                                                   uint32_t* __restrict__ dir_out, uint32_t* __restrict__ dir_n) {
  __shared__ uint32_t s_wave[16];
  __shared__ uint32_t s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  for (uint32_t base = 0; base < nb; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    uint32_t v = 0u, r = 0xffffffffu;
    if (i < nb) {
      const uint2 d = dir_in[i];
      r = d.x;
      v = r != 0xffffffffu ? 3u * W.block_tri[r] : d.y;
    }
    uint32_t xs = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t ys = __shfl_up(xs, o);
      if (lane >= (uint32_t)o) xs += ys;
    }
    if (lane == 63) s_wave[wave] = xs;
    __syncthreads();
    uint32_t add = s_carry;
    for (uint32_t w = 0; w < wave; ++w) add += s_wave[w];
    if (i < nb) {
      dir_out[i] = add + xs - v;
      dir_n[i] = v;
      if (r != 0xffffffffu) W.rb_first[r] = add + xs - v;
    }
    __syncthreads();
    if (threadIdx.x == 1023) s_carry = add + xs;
    __syncthreads();
  }
  if (threadIdx.x == 0) dir_out[nb] = s_carry;
}

// kept segments: moves[j] = {first vertex in the old arena, first vertex in the new one, vertices}
__global__ void __launch_bounds__(256) k_mesh_copy(MeshArena from, MeshArena to, const uint32_t* __restrict__ moves) {
  const uint32_t src = moves[3 * blockIdx.x], dst = moves[3 * blockIdx.x + 1], n = moves[3 * blockIdx.x + 2];
  for (uint32_t i = threadIdx.x; i < 3u * n; i += 256u) {
    to.xyz[3 * (size_t)dst + i] = from.xyz[3 * (size_t)src + i];
    to.nrm[3 * (size_t)dst + i] = from.nrm[3 * (size_t)src + i];
  }
  for (uint32_t i = threadIdx.x; i < n; i += 256u) {
    to.rgba[(size_t)dst + i] = from.rgba[(size_t)src + i];
    to.label[(size_t)dst + i] = from.label[(size_t)src + i];
  }
}

}  // namespace ksk
