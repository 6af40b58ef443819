// ks_k_shard_merged.h — the EXACT frame-sharded integration of `merged` (ks_integrate_round_exact, include/ks_hip.h;
// the scheme itself: ks_k_shard.h).
//
// `merged` builds its bundle maps afresh for every frame ([K:src/semantic_tsdf_integrator_merged.cpp:97-149]) and has no
// approximate sets: a frame's bundling, bundle order, ray casting, anti-grazing test and clearing pass depend on nothing but
// the frame.  A marcher therefore integrates no empty frames for the other ranks, and no voxel couples frames.
//
// What differs from `fast` is what an update carries.  The TSDF operands come from the bundle's MERGED point and weight
// (RayDesc at the bundle's first-point position — k_shard_export reads exactly that for method = merged), and the semantic
// increment is per bundle: { d_match, d_non } for a pure-label bundle, a 21-float vector for a mixed-label one.  They reach
// the owner as the marcher computed them, through two tables per frame:
//
//   record        unchanged, 20 bytes: { tile key << 9 | voxel in tile, info byte << 24 | BUNDLE NUMBER, sdf, update weight }
//                 (the marcher numbers the bundles that have at least one update 0 .. n_bundles - 1; the info byte is
//                 label | kind << 5 | clearing << 7 as in the pair keys)
//   bundle table  8 bytes per bundle, by bundle number: { d_match, d_non }; for a mixed-label bundle the first word is the
//                 bundle's row in the mixed table (an integer), the second is unused
//   mixed table   84 bytes (21 f32) per mixed-label bundle
//
// Both tables go to every peer that receives a record of the frame, whole, once (a 640x480 frame: ~21 000 bundles = 170 KB,
// ~1 900 mixed = 160 KB, next to ~95 MB of records in all: without an early-out a frame has 4.8 M updates).  The bundle numbers are handed out by wave-level appends: their
// order on the wire is not fixed, what a number names is.
//
// Owner side.  Every bundle's ray starts at the sensor, so the voxels next to it collect one update per bundle: runs of
// 1e4 (160x120) to 1e5 (1280x720) updates, where `fast` with the early-out has runs of a few.  After the stable sort by voxel
//   k_shard_stage_merged       lane per update: the operands in run order, { sdf, uw, bundle-table entry } as one 16-byte
//                              word (the update kernels then read sequentially, no indirection on the recurrences' path),
//                              and the heads of the runs of more than kLongRun updates, listed
//   k_shard_apply_merged       lane per run of at most kLongRun updates
//   k_shard_apply_merged_long  a listed run is taken by TWO wavefronts that share nothing: one walks the TSDF recurrence
//                              (dwords 0, 1 of the record), the other the 21 class sums in lanes 0 .. 20, the label and the
//                              colour (dwords 2 .. 25; with the colour taken from the labels it does not depend on the
//                              TSDF half).  Both load the operands 64 updates at a time, coalesced, one batch ahead; the TSDF
//                              half hands them across the lanes with v_readlane, the semantic half through a 64 x 21 block of
//                              increments in LDS (mixed-label vectors fetched straight from the table by their update's lane).
// The threshold is the one-GPU path's (kLongRun = 32): a wavefront pays one round trip to memory per 64 updates where a lane
// pays one per update, hidden only by the other lanes' runs; at about half a batch the two cost the same, and the lane
// kernel's longest walk stays at 32 steps.  Every sum advances strictly in update order, as in k_shard_apply.
#pragma once
#include "ks_k_shard.h"

namespace ksk {

constexpr uint32_t kShardSeqMask = (1u << kShardSeqBits) - 1u;
__device__ __forceinline__ uint32_t shard_min(uint32_t a, uint32_t b) { return a < b ? a : b; }   // (n < 2^31: no wrap-around)

// ---- marcher -------------------------------------------------------------------------------------------------------
// Which positions are bundles with at least one update (same-value stores: benign).
__global__ void __launch_bounds__(256) k_shard_mark_bundles(unsigned long long n_pairs, const uint32_t* __restrict__ seq,
                                                            uint32_t* __restrict__ bundle_no) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i < n_pairs) bundle_no[seq[i] & kShardSeqMask] = 1u;
}

// Lane per point position: a marked one gets its bundle number and its table entry; a mixed-label one a row as well.
// cnt[0] = bundles, cnt[1] = mixed-label bundles.
__global__ void __launch_bounds__(256) k_shard_bundle_table(uint32_t n, const RayDesc* __restrict__ rays, uint32_t* __restrict__ bundle_no,
                                                            float2* __restrict__ btab, uint32_t* __restrict__ mixed_pos,
                                                            uint32_t* __restrict__ cnt) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  const bool used = p < n && bundle_no[p] == 1u;
  uint4 d1 = make_uint4(0u, 0u, 0u, 0u);
  if (used) d1 = ((const uint4*)rays)[(size_t)p * 2 + 1];   // merged: the descriptor sits at the bundle's first position
  const bool mixed = used && ((d1.w >> 8) & 3u) == 2u;
  const uint32_t b = wave_append(used, &cnt[0]);
  const uint32_t row = wave_append(mixed, &cnt[1]);
  if (!used) return;
  bundle_no[p] = b;
  btab[b] = mixed ? make_float2(__uint_as_float(row), 0.0f) : make_float2(__uint_as_float(d1.y), __uint_as_float(d1.z));
  if (mixed) mixed_pos[row] = p;
}

// The 21-float vectors of the mixed-label bundles, compacted (deltas is indexed by first-point position).
__global__ void __launch_bounds__(256) k_shard_mixed_rows(uint32_t n_mixed, const uint32_t* __restrict__ mixed_pos,
                                                          const float* __restrict__ deltas, float* __restrict__ out) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n_mixed * (uint32_t)kNumLabels) return;
  const uint32_t row = e / (uint32_t)kNumLabels, l = e - row * (uint32_t)kNumLabels;
  out[e] = deltas[(size_t)mixed_pos[row] * kNumLabels + l];
}

// k_shard_gather with the position replaced by the bundle number.
__global__ void __launch_bounds__(256) k_shard_gather_merged(unsigned long long n, const uint64_t* __restrict__ okey_sorted,
                                                             const uint64_t* __restrict__ gkey, const uint32_t* __restrict__ seq,
                                                             const float* __restrict__ sdf, const float* __restrict__ uw,
                                                             const uint32_t* __restrict__ bundle_no, uint64_t* __restrict__ gkey_o,
                                                             uint32_t* __restrict__ seq_o, float* __restrict__ sdf_o, float* __restrict__ uw_o) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i >= n) return;
  const unsigned long long j = okey_sorted[i] & 0x00ffffffffffffffull;
  const uint32_t s = seq[j];
  gkey_o[i] = gkey[j];
  seq_o[i] = (s & ~kShardSeqMask) | bundle_no[s & kShardSeqMask];
  sdf_o[i] = sdf[j];
  uw_o[i] = uw[j];
}

// ---- owner ---------------------------------------------------------------------------------------------------------
// pairs: [63:56] info byte | voxel << 24 | bundle number, stably sorted by voxel (k_shard_import, the sort of shard_apply_segment).
__global__ void __launch_bounds__(256) k_shard_stage_merged(uint32_t n, uint32_t n_bundles, const uint64_t* __restrict__ pairs,
                                                            const uint32_t* __restrict__ vals, const float* __restrict__ sdf_in,
                                                            const float* __restrict__ uw_in, const float2* __restrict__ btab,
                                                            float4* __restrict__ ops, uint32_t* __restrict__ long_list,
                                                            uint32_t* __restrict__ n_long) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool is_long = false;
  if (i < n) {
    const uint64_t key = pairs[i];
    const uint32_t vox = (uint32_t)(key >> kShardSeqBits);
    const uint32_t r = vals[i];
    const uint32_t b = (uint32_t)key & kShardSeqMask;
    const float2 e = b < n_bundles ? btab[b] : make_float2(0.0f, 0.0f);   // (a record can only name a bundle of its frame's table)
    ops[i] = make_float4(sdf_in[r], uw_in[r], e.x, e.y);
    const bool head = i == 0u || (uint32_t)(pairs[i - 1] >> kShardSeqBits) != vox;
    is_long = head && i + kLongRun < n && (uint32_t)(pairs[i + kLongRun] >> kShardSeqBits) == vox;
  }
  const uint32_t at = wave_append(is_long, n_long);
  if (is_long) long_list[at] = i;
}

// label = first strict maximum, colour, the `updated` mark: how k_shard_apply ends
template <int COLOR_MODE>
__device__ __forceinline__ uint32_t shard_label_color(uint32_t bi, float bv, const uint32_t* __restrict__ label_lut) {
  if (COLOR_MODE == KS_COLOR_MODE_SEMANTIC) return label_lut[bi & 255u];
  return rainbow_color_map((double)(float)exp((double)bv));
}

// A lane per run of at most kLongRun updates.
template <int COLOR_MODE>
__global__ void __launch_bounds__(256) k_shard_apply_merged(TsdfParams Pm, uint32_t n, uint32_t n_mixed, const uint64_t* __restrict__ pairs,
                                                            const float4* __restrict__ ops, const float* __restrict__ mixed, Pool P,
                                                            const uint32_t* __restrict__ label_lut) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t vox = (uint32_t)(pairs[i] >> kShardSeqBits);
  if (i > 0 && (uint32_t)(pairs[i - 1] >> kShardSeqBits) == vox) return;                               // not the head of its run
  if (i + kLongRun < n && (uint32_t)(pairs[i + kLongRun] >> kShardSeqBits) == vox) return;            // k_shard_apply_merged_long's
  uint32_t* rec = (uint32_t*)(P.vox + (size_t)vox * 8);
  float dist = __uint_as_float(rec[0]), weight = __uint_as_float(rec[1]);
  uint32_t color = rec[2];
  float p[kNumLabels];
#pragma unroll
  for (int l = 0; l < kNumLabels; ++l) p[l] = __uint_as_float(rec[4 + l]);
  for (uint32_t j = i; j < n; ++j) {
    const uint64_t key = pairs[j];
    if ((uint32_t)(key >> kShardSeqBits) != vox) break;
    const float4 u = ops[j];
    tsdf_combine<false>(Pm, u.x, u.y, 0u, dist, weight, color);
    const uint32_t b = (uint32_t)(key >> 56);
    const uint32_t kind = (b >> 5) & 3u, lab = b & 0x1fu;
    if (kind == 1u) {
#pragma unroll
      for (int l = 0; l < kNumLabels; ++l) p[l] += ((uint32_t)l == lab) ? u.z : u.w;
    } else if (kind == 2u) {
      const uint32_t row = __float_as_uint(u.z);
      if (row < n_mixed) {
        const float* dl = mixed + (size_t)row * kNumLabels;
#pragma unroll
        for (int l = 0; l < kNumLabels; ++l) p[l] += dl[l];
      }
    }
  }
  float bv = p[0];
  uint32_t bi = 0u;
#pragma unroll
  for (int l = 1; l < kNumLabels; ++l)
    if (p[l] > bv) {
      bv = p[l];
      bi = (uint32_t)l;
    }
  color = shard_label_color<COLOR_MODE>(bi, bv, label_lut);
  rec[0] = __float_as_uint(dist);
  rec[1] = __float_as_uint(weight);
  rec[2] = color;
  rec[3] = bi;
#pragma unroll
  for (int l = 0; l < kNumLabels; ++l) rec[4 + l] = __float_as_uint(p[l]);
  rec[25] = 1u;  // updated since the last voxel-level host sync
}

// Workgroups of ONE wavefront; workgroup 2 r takes the TSDF half of listed run r, workgroup 2 r + 1 its semantic half.
// What bounds a run of 1e4 .. 1e5 updates is the length of the dependent chain per update, so both halves keep everything that does
// not depend on the voxel's state off that chain, the way k_apply_long does (ks_k_apply.h; same operations on the same operands in
// the same order, hence the same bits):
//   TSDF      per batch of 64: the weight recurrence first (add, compare, min — or nothing at all once the weight sits at
//             max_weight and no update weight is negative), then per LANE the reciprocal of its update's new weight and the
//             product sdf * uw, then the distance recurrence with a correctly rounded division by that reciprocal
//             (div_by_recip) — skipped while the distance sits at +truncation and every update of the batch keeps it there
//   semantic  per batch: lane j writes the 21 increments of update j to LDS (a pure-label bundle's { d_match, d_non } spread by
//             label, a mixed-label bundle's vector from the table, -0.0f — the one addend that changes no float — for an update
//             without a label), then lane l folds column l in, strictly in update order: 64 LDS reads in flight, 64 adds
template <int COLOR_MODE>
__global__ void __launch_bounds__(64) k_shard_apply_merged_long(TsdfParams Pm, uint32_t n, uint32_t n_mixed, const uint64_t* __restrict__ pairs,
                                                                const float4* __restrict__ ops, const float* __restrict__ mixed, Pool P,
                                                                const uint32_t* __restrict__ label_lut,
                                                                const uint32_t* __restrict__ long_list, const uint32_t* __restrict__ n_long) {
  __shared__ float s_inc[64][kNumLabels];   // class increments of the batch's updates (stride 21 words: no bank conflicts)
  const uint32_t lane = threadIdx.x;
  const int cls = lane < (uint32_t)kNumLabels ? (int)lane : 0;
  const uint32_t n_tasks = 2u * *n_long;
  const uint32_t last = n - 1u;
  for (uint32_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
    const uint32_t start = long_list[task >> 1];
    const uint32_t vox = (uint32_t)(pairs[start] >> kShardSeqBits);
    uint32_t* rec = (uint32_t*)(P.vox + (size_t)vox * 8);
    // one batch ahead; every load of the pipeline is unconditional (index clamped)
    uint32_t base = start;
    uint64_t key_n = pairs[shard_min(base + lane, last)];
    float4 op_n = ops[shard_min(base + lane, last)];
    if ((task & 1u) == 0u) {
      // ---- the TSDF recurrence (tsdf_combine<false>, update by update) ----
      float dist = __uint_as_float(rec[0]), weight = __uint_as_float(rec[1]);
      for (;;) {
        const uint64_t key = key_n;
        const float4 op = op_n;
        const bool in = base + lane < n && (uint32_t)(key >> kShardSeqBits) == vox;
        const int cnt = (int)__popcll(__ballot(in));   // sorted: the lanes of the run form a prefix
        key_n = pairs[shard_min(base + 64u + lane, last)];
        op_n = ops[shard_min(base + 64u + lane, last)];
        const float sdf = in ? op.x : 0.0f, uw = in ? op.y : 0.0f;
        // pass 1: w' = min(max_weight, w + uw) unless w + uw < 1e-6 (then the update is a no-op)
        float my_w = 0.0f, my_nw = 1.0f;
        if (weight == Pm.max_weight && __ballot(in && !(uw >= 0.0f)) == 0ull) {
          my_w = weight;   // every update sees w = max_weight and leaves it there
          my_nw = weight + uw;
        } else {
          float w_run = weight;
          for (int k = 0; k < cnt; ++k) {
            const float nw = w_run + bcast_f(uw, k);
            if ((int)lane == k) {
              my_w = w_run;
              my_nw = nw;
            }
            if (!(nw < kEps)) w_run = std_min(Pm.max_weight, nw);
          }
          weight = w_run;
        }
        const bool my_skip = my_nw < kEps;
        const float my_r = 1.0f / my_nw;   // correctly rounded, off the chain
        const float my_p = sdf * uw;
        // at +truncation, an update whose weighted mean exceeds the truncation by more than the rounding slack leaves it there
        const bool my_sat = my_skip || ((sdf - Pm.trunc) * uw >= 1e-6f * Pm.trunc * my_nw);
        const bool all_sat = __ballot(in && !my_sat) == 0ull;
        if (!(all_sat && dist == Pm.trunc)) {
          // pass 2: d' = clamp((sdf * uw + d * w) / (w + uw))
          for (int k = 0; k < cnt; ++k) {
            if (bcast_u(my_skip ? 1u : 0u, k)) continue;
            const float num = bcast_f(my_p, k) + dist * bcast_f(my_w, k);
            const float q = div_by_recip(num, bcast_f(my_nw, k), bcast_f(my_r, k));
            dist = (q > 0.0f) ? std_min(Pm.trunc, q) : std_max(-Pm.trunc, q);
          }
        }
        if (cnt < 64) break;
        base += 64u;
      }
      if (lane == 0u) {
        rec[0] = __float_as_uint(dist);
        rec[1] = __float_as_uint(weight);
      }
      continue;
    }
    // ---- the 21 class sums: lane l owns class l, every sum strictly in update order ----
    float pri = lane < (uint32_t)kNumLabels ? __uint_as_float(rec[4 + lane]) : 0.0f;
    for (;;) {
      const uint64_t key = key_n;
      const float4 op = op_n;
      const bool in = base + lane < n && (uint32_t)(key >> kShardSeqBits) == vox;
      const int cnt = (int)__popcll(__ballot(in));
      key_n = pairs[shard_min(base + 64u + lane, last)];
      op_n = ops[shard_min(base + 64u + lane, last)];
      if (in) {
        const uint32_t info = (uint32_t)(key >> 56);
        const uint32_t kind = (info >> 5) & 3u, lab = info & 0x1fu;
        const uint32_t row = __float_as_uint(op.z);
        if (kind == 2u && row < n_mixed) {
          const float* dl = mixed + (size_t)row * kNumLabels;
#pragma unroll
          for (int l = 0; l < kNumLabels; ++l) s_inc[lane][l] = dl[l];
        } else {
          const float a = kind == 1u ? op.z : -0.0f, b = kind == 1u ? op.w : -0.0f;   // (x + -0.0f == x for every x, -0.0f included)
#pragma unroll
          for (int l = 0; l < kNumLabels; ++l) s_inc[lane][l] = ((uint32_t)l == lab) ? a : b;
        }
      }
      __syncthreads();
      if (cnt == 64) {
        float x[64];   // all 64 increments are requested before the first dependent add
#pragma unroll
        for (int k = 0; k < 64; ++k) x[k] = s_inc[k][cls];
#pragma unroll
        for (int k = 0; k < 64; ++k) pri += x[k];
      } else {
#pragma unroll 8
        for (int k = 0; k < cnt; ++k) pri += s_inc[k][cls];
      }
      __syncthreads();   // the batch has been read: the next one may overwrite it
      if (cnt < 64) break;
      base += 64u;
    }
    // first strict maximum over lanes 0 .. 20
    uint32_t best = 0u;
    float m = bcast_f(pri, 0);
#pragma unroll
    for (int l = 1; l < kNumLabels; ++l) {
      const float x = bcast_f(pri, l);
      if (x > m) {
        m = x;
        best = (uint32_t)l;
      }
    }
    if (lane < (uint32_t)kNumLabels) rec[4 + lane] = __float_as_uint(pri);
    if (lane == 0u) {
      rec[2] = shard_label_color<COLOR_MODE>(best, m, label_lut);
      rec[3] = best;
      rec[25] = 1u;  // updated since the last voxel-level host sync
    }
  }
}

}  // namespace ksk
