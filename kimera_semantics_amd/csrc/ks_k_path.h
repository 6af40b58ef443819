// ks_k_path.h — ks_path_shorten: a polyline pulled taut by line of sight over the stored ESDF.  The contract (the greedy rule, the
// chunks of 64 candidates from the far end, the outputs and the eight sums) is DESIGN.md, section "Path shortening";
// tests/path_shorten_model.py restates it on tests/esdf_read_model.py's sweep and the kernel is compared with it bit for bit.
//
//   k_path_shorten   one wavefront per path, four per workgroup, paths in a grid-stride loop.  The anchor P[a] is wave-uniform; lane l
//                    of chunk c sweeps the candidate hi - 64 c - l with the walk of k_esdf_sweep (path_sweep below restates its
//                    twenty lines: factoring them out of k_esdf_sweep changed that kernel's instruction stream).  One ballot of
//                    FREE per chunk; the LOWEST set lane holds the farthest free candidate.  Its length and clearance go to all
//                    lanes by __shfl, lane 0 stores the row.  A wavefront runs as long as the longest sweep of a chunk: far
//                    candidates take more samples than near ones, which is the known cost of this shape.
// The store is only read.  No LDS, no floating-point atomics: a wavefront keeps its eight sums and adds each with one integer atomic
// when it has no path left.
#pragma once
#include "ks_k_esdf_read.h"

namespace ksk {

struct PathShorten {
  const float* in;             // [n][max_waypoints][3]
  const uint32_t* n_in;        // [n]
  size_t n;
  uint32_t max_waypoints, lookahead;
  float radius, min_step, max_length;   // as EsdfSweep
  int32_t unknown_is_free, max_samples;
  uint8_t* status;             // [n]   any of the five may be nullptr
  uint32_t* n_out;             // [n]
  float* out;                  // [n][max_waypoints][3]; may be `in`: row k <= a is written after every read of the rows below a
  float* length;               // [n]
  float* min_clearance;        // [n]
  unsigned long long* counters;   // ok | unverified | invalid | waypoints_in | waypoints_out | segments_unverified | sweeps | samples
};

// SW(a, b): the walk of k_esdf_sweep (ks_k_esdf_read.h), operation for operation: a change to either copy goes into both.  Returns the
// status; L also for an INVALID segment.
__device__ __forceinline__ uint32_t path_sweep(const TileTable& T, const EsdfReadStore& S, TileMemo& M, const PathShorten& W, float ax, float ay, float az,
                                               float bx, float by, float bz, float& L, float& min_c, int& samples) {
  const float inf = __uint_as_float(0x7f800000u);
  uint32_t status = 3u;   // KS_SWEEP_INVALID
  const float dx = bx - ax, dy = by - ay, dz = bz - az;
  L = sqrtf((dx * dx + dy * dy) + dz * dz);
  min_c = inf;
  if (L < inf && !(L > W.max_length)) {   // (the coordinates are finite: the path passed the finite test)
    const bool point = L == 0.0f;
    const float ux = point ? 0.0f : dx / L, uy = point ? 0.0f : dy / L, uz = point ? 0.0f : dz / L;
    float t = 0.0f;
    for (int it = 0; it < W.max_samples; ++it) {
      const EsdfSampleValue E = esdf_read_sample<false>(T, S, M, ax + t * ux, ay + t * uy, az + t * uz);
      ++samples;
      if (E.status == 0u && !W.unknown_is_free) {
        status = 2u;   // KS_SWEEP_UNKNOWN
        break;
      }
      float c = 0.0f;
      if (E.status != 0u) {
        c = E.distance - W.radius;
        if (c < min_c) min_c = c;
        if (c < 0.0f) {
          status = 1u;   // KS_SWEEP_COLLISION
          break;
        }
      }
      if (t >= L) {
        status = 0u;   // KS_SWEEP_FREE
        break;
      }
      const float step = E.status != 0u ? fmaxf(c, W.min_step) : W.min_step;
      t = fminf(t + step, L);
    }
    if (status == 3u) min_c = inf;   // (the bound)
  }
  return status;
}

// a value every lane of the wavefront holds, where the compiler can see that
__device__ __forceinline__ uint32_t path_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float path_uniform(float v) { return __uint_as_float(path_uniform(__float_as_uint(v))); }

// grid min(ceil(n / 4), the context's bound), 256 work-items: wavefront w of the grid takes the paths w, w + 4 gridDim.x, ...
__global__ void __launch_bounds__(256) k_path_shorten(TileTable T, EsdfReadStore S, PathShorten W) {
  const uint32_t lane = lane_id();
  const uint32_t wave = path_uniform((uint32_t)(threadIdx.x >> 6));
  const size_t stride = (size_t)gridDim.x * 4u;
  const float inf = __uint_as_float(0x7f800000u);
  // the wavefront's sums: all but c_samples are the same in every lane
  uint32_t c_ok = 0, c_unverified = 0, c_invalid = 0, c_segments = 0;
  unsigned long long c_in = 0, c_out = 0, c_sweeps = 0;
  unsigned long long c_samples = 0;   // this lane's
  TileMemo M;
  for (size_t i = (size_t)blockIdx.x * 4u + wave; i < W.n; i += stride) {
    const uint32_t m = path_uniform(W.n_in[i]);
    const float* P = W.in + i * (size_t)W.max_waypoints * 3u;
    float* Q = W.out ? W.out + i * (size_t)W.max_waypoints * 3u : nullptr;
    bool bad = m == 0u || m > W.max_waypoints;
    if (!bad) {                // lanes stride over the rows, one ballot decides
      bool odd = false;
      for (uint32_t r = lane; r < m; r += 64u) {
        const float x = P[3u * r], y = P[3u * r + 1u], z = P[3u * r + 2u];
        odd = odd || !(fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf);
      }
      bad = __ballot(odd) != 0ull;
    }
    uint32_t status = 2u, k = 0u;   // KS_SHORTEN_INVALID
    float length = 0.0f, min_clearance = inf;
    if (!bad) {
      status = 0u;             // KS_SHORTEN_OK
      float ax = path_uniform(P[0]), ay = path_uniform(P[1]), az = path_uniform(P[2]);
      if (Q && lane == 0u) {
        Q[0] = ax;
        Q[1] = ay;
        Q[2] = az;
      }
      k = 1u;
      uint32_t a = 0u;
      while (a < m - 1u) {
        const uint32_t hi = a + W.lookahead < m - 1u ? a + W.lookahead : m - 1u;
        uint32_t j_star = a + 1u;
        bool verified = false;
        float L_star = 0.0f, c_star = inf;
        // chunk c = 0, 1, ...: the candidates top - 63 .. top, top = hi - 64 c, clipped below at a + 1
        for (uint32_t top = hi;; top -= 64u) {
          const uint32_t count = top - a < 64u ? top - a : 64u;
          const bool has = lane < count;
          uint32_t st = 3u;
          float L = 0.0f, mc = inf;
          if (has) {
            const uint32_t j = top - lane;
            int samples = 0;
            st = path_sweep(T, S, M, W, ax, ay, az, P[3u * j], P[3u * j + 1u], P[3u * j + 2u], L, mc, samples);
            c_samples += (unsigned long long)(uint32_t)samples;
          }
          c_sweeps += count;
          const unsigned long long free = __ballot(has && st == 0u);
          const bool last = top - a <= 64u;
          if (free != 0ull || last) {
            // the farthest FREE candidate is in the lowest set lane; with none in any chunk, the input's own segment a -> a + 1
            const uint32_t src = free != 0ull ? (uint32_t)(__ffsll((long long)free) - 1) : top - (a + 1u);
            verified = free != 0ull;
            j_star = top - src;
            L_star = __shfl(L, (int)src);
            c_star = __shfl(mc, (int)src);
            break;
          }
        }
        if (!verified) {
          status = 1u;         // KS_SHORTEN_UNVERIFIED
          ++c_segments;
        }
        length = length + L_star;
        if (c_star < min_clearance) min_clearance = c_star;
        // the new anchor: read before row k is written (in place, k == j_star writes the bits that are there)
        ax = path_uniform(P[3u * j_star]);
        ay = path_uniform(P[3u * j_star + 1u]);
        az = path_uniform(P[3u * j_star + 2u]);
        if (Q && lane == 0u) {
          Q[3u * k] = ax;
          Q[3u * k + 1u] = ay;
          Q[3u * k + 2u] = az;
        }
        ++k;
        a = j_star;
      }
      c_in += m;
      c_out += k;
    }
    c_ok += status == 0u;
    c_unverified += status == 1u;
    c_invalid += status == 2u;
    if (lane == 0u) {
      if (W.status) W.status[i] = (uint8_t)status;
      if (W.n_out) W.n_out[i] = k;
      if (W.length) W.length[i] = length;
      if (W.min_clearance) W.min_clearance[i] = min_clearance;
    }
  }
  for (int off = 32; off >= 1; off >>= 1) c_samples += __shfl_xor(c_samples, off);
  if (lane == 0u) {
    if (c_ok) atomicAdd(&W.counters[0], (unsigned long long)c_ok);
    if (c_unverified) atomicAdd(&W.counters[1], (unsigned long long)c_unverified);
    if (c_invalid) atomicAdd(&W.counters[2], (unsigned long long)c_invalid);
    if (c_in) atomicAdd(&W.counters[3], c_in);
    if (c_out) atomicAdd(&W.counters[4], c_out);
    if (c_segments) atomicAdd(&W.counters[5], (unsigned long long)c_segments);
    if (c_sweeps) atomicAdd(&W.counters[6], c_sweeps);
    if (c_samples) atomicAdd(&W.counters[7], c_samples);
  }
}

}  // namespace ksk
