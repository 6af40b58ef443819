// ks_k_mesh_index.h — the indexed view of the stored mesh: shared vertices, a smooth normal per vertex, built from the mesh
// arena alone (ks_k_mesh.h: three corners per triangle, nothing shared).  The contract (identity by bits, order by first
// corner, integer normal sums, lifetime) is DESIGN.md §18; tests/mesh_index_model.py restates it in NumPy and the kernels
// are compared with it byte for byte.
//
// The corners are grouped by the library's stable radix sort on the position bits, payload = corner number: z first,
// then the 64-bit (x, y).  After a stable sort the first element of a run of equal positions is the run's smallest corner.
//
//   k_mi_keys_z     key = bits of z, payload = corner number                       (sort 1: 32 bits)
//   k_mi_keys_xy    key = bits of (x, y) of the corner at each sorted place         (sort 2: 64 bits)
//   k_mi_heads      sorted place s starts a run: 1, else 0
//   (inclusive scan: the run number of every sorted place, k_mi_scan_*)
//   k_mi_first      per run its first corner; that corner is flagged in CORNER order
//   (inclusive scan of the corner flags: the vertex number of every first corner — vertices ascend by first corner)
//   k_mi_emit       indices[corner] = vertex; the corner's face normal enters the vertex's three int32 sums and its
//                   valence (integer atomics: the sums do not depend on the order); a first corner also writes the
//                   vertex's position, colour and label
//   k_mi_finish     per vertex: normal = sums / length, in place; the largest valence
//   (the object ids come from k_obj_query over the vertex positions, ks_k_objects.h)
//
// The scan is the plain three-launch one (partial sums of 2048-element slices, one workgroup over the partials, apply):
// the arrays are some 1e5..1e6 words and every launch here is latency bound.
#pragma once
#include "ks_types.h"
#include "ks_k_mesh.h"

namespace ksk {

constexpr uint32_t kMiSlice = 2048;   // elements of a scan slice: 256 work-items x 8

struct MeshIndexOut {   // the indexed mesh on the device (capacity: the corner count)
  float* xyz;           // [V][3]
  float* nrm;           // [V][3]  first the int32 sums, then the normals (k_mi_finish, in place)
  uint32_t* rgba;       // [V]
  uint8_t* label;       // [V]
  uint32_t* indices;    // [C]
  uint32_t* valence;    // [V] corners per vertex
};

__global__ void __launch_bounds__(256) k_mi_keys_z(const float* __restrict__ xyz, uint32_t n, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  key[i] = __float_as_uint(xyz[3 * (size_t)i + 2]);
  val[i] = i;
}

__global__ void __launch_bounds__(256) k_mi_keys_xy(const float* __restrict__ xyz, const uint32_t* __restrict__ perm, uint32_t n,
                                                    uint64_t* __restrict__ key) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n) return;
  const size_t c = perm[s];
  key[s] = ((uint64_t)__float_as_uint(xyz[3 * c]) << 32) | (uint64_t)__float_as_uint(xyz[3 * c + 1]);
}

__global__ void __launch_bounds__(256) k_mi_heads(const float* __restrict__ xyz, const uint32_t* __restrict__ perm, uint32_t n,
                                                  uint32_t* __restrict__ head) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n) return;
  uint32_t h = 1u;
  if (s) {
    const size_t a = perm[s - 1], b = perm[s];
    h = (__float_as_uint(xyz[3 * a]) != __float_as_uint(xyz[3 * b]) || __float_as_uint(xyz[3 * a + 1]) != __float_as_uint(xyz[3 * b + 1]) ||
         __float_as_uint(xyz[3 * a + 2]) != __float_as_uint(xyz[3 * b + 2]))
            ? 1u
            : 0u;
  }
  head[s] = h;
}

// ---- inclusive scan of n words, in place ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mi_scan_partial(const uint32_t* __restrict__ v, uint32_t n, uint32_t* __restrict__ partial) {
  __shared__ uint32_t s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * kMiSlice;
  uint32_t t = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t i = base + (uint32_t)k * 256u + threadIdx.x;
    if (i < n) t += v[i];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
  if (lane_id() == 0) atomicAdd(&s_sum, t);
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = s_sum;
}

// one workgroup: exclusive scan of the partial sums in place; the grand total -> *total
__global__ void __launch_bounds__(1024) k_mi_scan_top(uint32_t* __restrict__ partial, uint32_t nb, uint32_t* __restrict__ total) {
  __shared__ uint32_t s_wave[16];
  __shared__ uint32_t s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  for (uint32_t base = 0; base < nb; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? partial[i] : 0u;
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
    if (i < nb) partial[i] = add + xs - v;
    __syncthreads();
    if (threadIdx.x == 1023) s_carry = add + xs;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = s_carry;
}

// every work-item scans 8 neighbouring words; the work-items of the slice by wavefront scans and the waves' totals
__global__ void __launch_bounds__(256) k_mi_scan_apply(uint32_t* __restrict__ v, uint32_t n, const uint32_t* __restrict__ partial) {
  __shared__ uint32_t s_wave[4];
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  const uint32_t first = blockIdx.x * kMiSlice + threadIdx.x * 8u;
  uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0, x4 = 0, x5 = 0, x6 = 0, x7 = 0;
  if (first + 7u < n) {
    const uint4 a = *(const uint4*)(v + first), b = *(const uint4*)(v + first + 4);
    x0 = a.x; x1 = a.y; x2 = a.z; x3 = a.w; x4 = b.x; x5 = b.y; x6 = b.z; x7 = b.w;
  } else {
    if (first < n) x0 = v[first];
    if (first + 1u < n) x1 = v[first + 1];
    if (first + 2u < n) x2 = v[first + 2];
    if (first + 3u < n) x3 = v[first + 3];
    if (first + 4u < n) x4 = v[first + 4];
    if (first + 5u < n) x5 = v[first + 5];
    if (first + 6u < n) x6 = v[first + 6];
  }
  x1 += x0; x2 += x1; x3 += x2; x4 += x3; x5 += x4; x6 += x5; x7 += x6;
  uint32_t xs = x7;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t ys = __shfl_up(xs, o);
    if (lane >= (uint32_t)o) xs += ys;
  }
  if (lane == 63) s_wave[wave] = xs;
  __syncthreads();
  uint32_t add = partial[blockIdx.x] + xs - x7;
  for (uint32_t w = 0; w < wave; ++w) add += s_wave[w];
  x0 += add; x1 += add; x2 += add; x3 += add; x4 += add; x5 += add; x6 += add; x7 += add;
  if (first + 7u < n) {
    *(uint4*)(v + first) = make_uint4(x0, x1, x2, x3);
    *(uint4*)(v + first + 4) = make_uint4(x4, x5, x6, x7);
  } else {
    if (first < n) v[first] = x0;
    if (first + 1u < n) v[first + 1] = x1;
    if (first + 2u < n) v[first + 2] = x2;
    if (first + 3u < n) v[first + 3] = x3;
    if (first + 4u < n) v[first + 4] = x4;
    if (first + 5u < n) v[first + 5] = x5;
    if (first + 6u < n) v[first + 6] = x6;
  }
}

// run[s] = inclusive scan of the head flags: sorted place s belongs to run run[s] - 1
__global__ void __launch_bounds__(256) k_mi_first(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ run, uint32_t n,
                                                  uint32_t* __restrict__ first_corner, uint32_t* __restrict__ corner_flag) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n) return;
  const uint32_t r = run[s];
  if (s == 0 || run[s - 1] != r) {
    const uint32_t c = perm[s];
    first_corner[r - 1] = c;
    corner_flag[c] = 1u;
  }
}

// vertex_of[c] = inclusive scan of the corner flags: first corner c is vertex vertex_of[c] - 1
__global__ void __launch_bounds__(256) k_mi_emit(MeshArena A, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ run,
                                                 const uint32_t* __restrict__ first_corner, const uint32_t* __restrict__ vertex_of, uint32_t n,
                                                 MeshIndexOut O) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n) return;
  const size_t c = perm[s];
  const uint32_t fc = first_corner[run[s] - 1];
  const size_t v = vertex_of[fc] - 1u;
  O.indices[c] = (uint32_t)v;
  int* sums = (int*)O.nrm + 3 * v;
  atomicAdd(sums, (int)rintf(A.nrm[3 * c] * 65536.0f));
  atomicAdd(sums + 1, (int)rintf(A.nrm[3 * c + 1] * 65536.0f));
  atomicAdd(sums + 2, (int)rintf(A.nrm[3 * c + 2] * 65536.0f));
  atomicAdd(O.valence + v, 1u);
  if (c == (size_t)fc) {
    O.xyz[3 * v] = A.xyz[3 * c];
    O.xyz[3 * v + 1] = A.xyz[3 * c + 1];
    O.xyz[3 * v + 2] = A.xyz[3 * c + 2];
    O.rgba[v] = A.rgba[c];
    O.label[v] = A.label[c];
  }
}

// counts[0] = V (the total of the second scan), counts[1] = the largest valence (zeroed beforehand)
__global__ void __launch_bounds__(256) k_mi_finish(MeshIndexOut O, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_max;
  if (threadIdx.x == 0) s_max = 0;
  __syncthreads();
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v < counts[0]) {
    const int* sums = (const int*)O.nrm + 3 * (size_t)v;
    const float sx = (float)sums[0], sy = (float)sums[1], sz = (float)sums[2];
    const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
    const bool ok = len > 0.0f;
    O.nrm[3 * (size_t)v] = ok ? sx / len : 0.0f;
    O.nrm[3 * (size_t)v + 1] = ok ? sy / len : 0.0f;
    O.nrm[3 * (size_t)v + 2] = ok ? sz / len : 0.0f;
    atomicMax(&s_max, O.valence[v]);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_max) atomicMax(counts + 1, s_max);
}

}  // namespace ksk
