/*
 * ks_hip.h — C ABI of the MI355X-native semantic TSDF integrator (libks_hip.so).
 *
 * This is the drop-in boundary underneath the reference's plugin surface.  The only caller
 * in a Kimera-Semantics deployment is the host adapter class
 * (kimera_semantics_amd/host/hip_semantic_tsdf_integrator.h) which derives from
 * voxblox::TsdfIntegratorBase + kimera::SemanticIntegratorBase exactly like the two CPU
 * integrators it replaces, and is returned by SemanticTsdfIntegratorFactory::create
 * (kimera_semantics/src/semantic_tsdf_integrator_factory.cpp:43-88).  Plain pointers and
 * sizes only; no C++/torch types.  One ks_ctx per GPU; a ks_ctx is NOT thread-safe (the
 * reference calls integratePointCloud from one ROS spinner thread).
 *
 * All functions return 0 on success or a negative KS_ERR_* code; ks_last_error() gives
 * text.  Where the reference would CHECK-abort (glog), the C ABI returns an error and the
 * adapter turns it back into LOG(FATAL) to preserve the convention.
 */
#ifndef KS_HIP_H_
#define KS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KS_NUM_LABELS 21 /* kimera::kTotalNumberOfLabels, kimera_semantics/include/kimera_semantics/common.h:26 */

enum {
  KS_OK = 0,
  KS_ERR_INVALID_ARG = -1,
  KS_ERR_LABEL_RANGE = -2,   /* label >= 21: CHECK_LT at semantic_tsdf_integrator_fast.cpp:134 / merged.cpp:278 */
  KS_ERR_PROBABILITY = -3,   /* CHECKs of semantic_integrator_base.cpp:98-107 */
  KS_ERR_HIP = -4,           /* HIP runtime failure */
  KS_ERR_POOL_FULL = -5,     /* voxel-tile pool exhausted (raise ks_config.max_tiles) */
  KS_ERR_INDEX_RANGE = -6,   /* a voxel index left the +-2^23 range the device packs */
  KS_ERR_NO_DEVICE = -7,
  KS_ERR_UNSUPPORTED = -8,
  KS_ERR_PEER_FAILED = -9    /* a collective call: another rank failed (the text names it); nothing was applied on this rank */
};

enum { KS_METHOD_FAST = 0, KS_METHOD_MERGED = 1 };          /* factory names "fast"/"merged", semantic_tsdf_integrator_factory.h:49-54 */
enum { KS_COLOR_MODE_COLOR = 0, KS_COLOR_MODE_SEMANTIC = 1, KS_COLOR_MODE_SEMANTIC_PROBABILITY = 2 }; /* ColorMode, semantic_integrator_base.h:54-58 */
/* voxblox integration_order_mode (vxb::ThreadSafeIndexFactory::get, called at semantic_tsdf_integrator_fast.cpp:172-174 and
 * semantic_tsdf_integrator_merged.cpp:115-117).  Voxblox is not part of the reference tree (un-pinned upstream), so the
 * permutation behind "mixed" cannot be read there; both readings of MixedThreadSafeIndex::getNextIndexImpl are implemented,
 * with q = N / 1024 and positions s >= q * 1024 mapping to themselves:
 *   KS_ORDER_MIXED             idx = (s % q) * 1024 + s / q     upstream as published (number_of_groups_ = N / step_size_,
 *                              group_num = s % number_of_groups_, position_in_group = s / number_of_groups_)
 *   KS_ORDER_MIXED_1024_GROUPS idx = (s % 1024) * q + s / 1024  (what rounds 1-4 of this library assumed)
 * The C++ adapter does not guess: it reads the sequence of the ThreadSafeIndexFactory it is compiled against and selects
 * the matching value, or aborts (host/hip_semantic_tsdf_integrator.cpp: probe_mixed_order). */
enum { KS_ORDER_MIXED = 0, KS_ORDER_SORTED = 1, KS_ORDER_MIXED_1024_GROUPS = 2 };
/* merged: the order the ray bundles are integrated in.
 * REFERENCE (default): the iteration order of the libstdc++ std::unordered_map the reference keeps them in
 *   (semantic_tsdf_integrator_merged.cpp:108-124, 200-232; VoxelMap, common.h:37) — what the reference does at
 *   integrator_threads = 1, reproduced on the GPU from the keys' insertion order, hash codes and the container's
 *   rehash schedule (csrc/ks_k_bundle_order.h): results are bit-identical to the reference's.
 * CANONICAL: first-insertion order (a container-independent order; a few launches cheaper per frame). */
enum { KS_BUNDLE_ORDER_REFERENCE = 0, KS_BUNDLE_ORDER_CANONICAL = 1 };
enum { KS_EARLY_OUT_EXACT = 1 };                             /* value of ks_config.early_out_phase_growth, see there */

/* voxblox::TsdfIntegratorBase::Config + kimera SemanticIntegratorBase::SemanticConfig
 * (semantic_integrator_base.h:68-87) + layer geometry + device sizing, as one POD.
 * The first block of fields is laid out exactly like the oracle's ko_config so tests can
 * fill both from one dict. */
typedef struct ks_config {
  float voxel_size;
  int32_t voxels_per_side;          /* host Layer block edge (8, 16, 32 or 64); device tiles are always 8^3 */
  float truncation_distance;
  float max_weight;
  float min_ray_length_m;
  float max_ray_length_m;
  int32_t voxel_carving_enabled;
  int32_t use_const_weight;
  int32_t allow_clear;
  int32_t use_weight_dropoff;
  int32_t use_sparsity_compensation_factor;
  float sparsity_compensation_factor;
  int32_t enable_anti_grazing;
  float start_voxel_subsampling_factor;
  int32_t max_consecutive_ray_collisions;
  int32_t clear_checks_every_n_frames;
  int32_t integration_order_mode;
  int32_t integrator_threads;       /* ignored on the GPU (kept for config compatibility) */
  int32_t method;
  int32_t bundle_order;             /* KS_BUNDLE_ORDER_* (merged only) */
  float semantic_measurement_probability;
  int32_t color_mode;
  int32_t n_dynamic_labels;
  uint8_t dynamic_labels[32];
  uint8_t label_rgba[256][4];       /* label -> colour (SemanticLabel2Color::semantic_label_to_color_map_) */
  /* fast integrator with the early-out enabled (max_consecutive_ray_collisions below the ray length):
   * the reference's loop (semantic_tsdf_integrator_fast.cpp:110-122) is serial by construction — ray k
   * stops on the marks rays 1..k-1 left in the approximate set.
   * 0 (default) or KS_EARLY_OUT_EXACT: the reference's SERIAL result itself (what integrator_threads = 1 produces, bit
   *    for bit, including the ApproxHashSet's zero-initialised slots that "contain" hash 0).  The serial result is the
   *    unique fixed point of "how far does every ray get against the marks of the rays before it"; the GPU reaches it
   *    with an event-driven iteration on the device (csrc/ks_k_exact.h: the seed's marks sorted once, then only rays
   *    whose inputs changed are re-evaluated; no host read in the loop), pipelined like every other mode when
   *    clear_checks_every_n_frames = 1 (with a larger value a frame's marks are inputs of the next frame's loop:
   *    pipeline_frames is then treated as 0).  Long rays (more than 400 voxels: 2 cm voxels / 10 m rays): whole-ray marks
   *    sorted once, then sweeps along the chains of the integration order on the device; one frame at a time
   *    (pipeline_frames treated as 0), the host reads two words per dozen sweeps.
   * 16 .. 4096: the ORDERED-PHASE schedule alone (restated for the CPU in oracle/ks_oracle.cpp, against
   *    which it is bit-exact): integration positions are cut into phases whose length grows by this factor (in
   *    1/16ths) — 32 = doubling, 16 = one generation (one integration position per chain = per group of the integration order) per phase.  Deterministic for every value, a few
   *    launches cheaper per frame than the exact mode, and NOT the reference's map (touched-voxel Jaccard against the serial order, 640x480 / 5 cm, "mixed" order in upstream's
   *    form: 0.9998 for 16, 0.976 for 24, 0.962 for 32, 0.916 for 64 — DESIGN.md §3.2; tests/test_early_out_fidelity.py asserts >= 0.93 for 32): a throughput option for callers who accept that. */
  int32_t early_out_phase_growth;
  /* ---- device sizing ---- */
  int32_t device_id;                /* HIP device ordinal */
  uint32_t max_tiles;               /* INITIAL capacity of the 8^3-voxel tile pool (64 KiB each); the pool is doubled
                                       between frames whenever more than half of it is in use (the reference
                                       allocates blocks without a cap, semantic_integrator_base.cpp:205-254).
                                       KS_ERR_POOL_FULL remains for a single frame that needs more than the free half. */
  uint32_t max_points;              /* largest cloud per call (buffers grow on demand if exceeded) */
  /* 0 (default): an integrate call returns with its frame fully enqueued and its own statistics.
   * 1 .. 16: frame pipelining for streams of frames (bag replay): the value is how many calls the second
   *    half of a frame (pair sort + voxel update) lags behind.  A call enqueues stages A and B of its frame
   *    (points .. early-out phases and pair emission) and finishes the frame `pipeline_frames` calls back; the
   *    one host wait of a frame then overlaps GPU work of later frames, and stage B of up to four consecutive
   *    frames runs concurrently: on four streams (values below 8), or — values 8 .. 15 — as one batched launch sequence
   *    per four frames (every kernel of stage B covers the batch), or — value 16 — per eight frames.  Larger values
   *    keep the host further ahead at the price of that many frames of latency (and of frame slots: 12 up to 8, 24 above).
   *    The statistics a call returns are those of the frames completed since statistics were last
   *    returned (summed if several), i.e. they lag by `pipeline_frames` calls; so do KS_ERR_LABEL_RANGE /
   *    pool errors.  Every other entry point (queries, download, export, ks_synchronize, ks_flush)
   *    completes the outstanding frames first, so the map they see is the same as without
   *    pipelining. */
  int32_t pipeline_frames;
} ks_config;

typedef struct ks_frame_stats {
  uint64_t n_points;
  uint64_t n_valid_points;
  uint64_t n_rays_cast;        /* fast: points surviving start-voxel dedup; merged: bundles */
  uint64_t n_voxel_updates;    /* (ray, voxel) pairs applied = reference updateTsdfVoxel+updateSemanticVoxel calls */
  uint64_t n_blocks_allocated; /* new 8^3 device tiles this frame */
} ks_frame_stats;

/* Accumulated HIP-event timings per pipeline stage (enabled with ks_profile_enable). */
enum {
  KS_STAGE_POINTS = 0,   /* per-point validity/transform/keys */
  KS_STAGE_SORT_POINTS,  /* dedup / bundling sort */
  KS_STAGE_RAYS,         /* dedup decision or bundle merge */
  KS_STAGE_MARCH,        /* ONE DDA walk per ray: tile allocation, observed-set early-out, (voxel, ray) pair emission,
                            counter snapshot (k_march + k_publish) */
  KS_STAGE_EMIT,         /* start of the tail: initialisation of the tiles the march allocated (the name dates from a
                            two-pass march; kept for ABI stability) */
  KS_STAGE_SORT_PAIRS,   /* group pairs by voxel in ray order */
  KS_STAGE_APPLY,        /* k_apply: per-voxel TSDF + semantic log-likelihood update (runs < 32 updates) */
  KS_STAGE_APPLY_LONG,   /* k_apply_long: one wavefront per voxel with >= 32 updates */
  KS_STAGE_COUNT
};
typedef struct ks_profile {
  double ms[KS_STAGE_COUNT];       /* summed over profiled frames */
  uint64_t launches[KS_STAGE_COUNT];
  uint64_t frames;
  uint64_t updates;                /* voxel updates over profiled frames */
  uint64_t points;
  double apply_kernel_ms;          /* k_apply dispatch begin->end (hipExtLaunchKernel events), summed */
  uint64_t apply_kernel_launches;  /* ... over this many timed launches */
  uint64_t apply_kernel_updates;   /* ... which performed this many voxel updates */
  double host_ms;                  /* wall time spent inside the integrate calls (enqueue + wait) */
  double host_wait_ms;             /* ... of which blocked on the per-frame counter snapshot */
} ks_profile;

typedef struct ks_ctx ks_ctx;

int ks_default_config(ks_config* cfg);
int ks_create(const ks_config* cfg, ks_ctx** out);
void ks_destroy(ks_ctx* ctx);
const char* ks_last_error(ks_ctx* ctx); /* ctx may be NULL: returns the last create-time error */

/* colour -> label map (SemanticLabel2Color::color_to_semantic_label_, color.cpp:57-66);
 * keys are RGBA with the alpha the CSV holds.  Lookups force alpha to 255 like
 * semantic_tsdf_integrator_fast.cpp:157 / merged.cpp:87; unknown colours map to label 0
 * (color.cpp:72-81). */
int ks_set_color_to_label(ks_ctx* ctx, const uint8_t* rgba_keys, const uint8_t* labels, size_t n);

/* vxb::TsdfIntegratorBase::integratePointCloud(T_G_C, points_C, colors, freespace)
 * (override at semantic_tsdf_integrator_fast.h:82-86 / merged.h:70-73) and the label-aware
 * overload merged.h:82-86.  Host pointers.  T_G_C = {qw,qx,qy,qz,tx,ty,tz}.
 * labels == NULL -> labels are derived from rgba through the colour map (the reference's
 * serial host loop, fast.cpp:150-158).  rgba == NULL -> colours are (0,0,0,0) (what the
 * reference's merged colour overload effectively integrates, merged.cpp:70,92-93).
 * Lifetime of the host buffers: pageable memory is staged before the call returns and may be reused at once; page-locked
 * memory (ks_host_alloc, hipHostMalloc, hipHostRegister) is read by the copy engine and may still be in use when a call of
 * a PIPELINED context returns (pipeline_frames = 0: the call completes its frame, the buffer is free): leave it unchanged
 * until `pipeline_frames` further integrate calls have returned (the call that finishes a frame has waited for it), or
 * until a call that completes outstanding work (ks_synchronize, ks_flush, any query) — i.e. rotate pipeline_frames + 1
 * buffers. */
int ks_integrate_points(ks_ctx* ctx, const float T_G_C[7], const float* xyz, const uint8_t* rgba,
                        const uint8_t* labels, size_t n, int freespace, ks_frame_stats* stats);
/* Same, but xyz/rgba/labels are DEVICE pointers already resident in HBM (bench timed region). */
int ks_integrate_points_device(ks_ctx* ctx, const float T_G_C[7], const float* d_xyz, const uint8_t* d_rgba,
                               const uint8_t* d_labels, size_t n, int freespace, ks_frame_stats* stats);

/* Depth + label image entry: the step BEFORE the hot path fused into the
 * GPU frontend.  Replaces PointCloudFromDepth::convert
 * (kimera_semantics_ros/include/kimera_semantics_ros/depth_map_to_pointcloud.h:213-275) plus the
 * colour->label host loop: back-projects with K = {fx, fy, cx, cy}, drops invalid pixels in image
 * order, then integrates exactly as ks_integrate_points would on the resulting cloud.
 * depth_fmt 0 = float32 metres (invalid: non-finite), 1 = uint16 millimetres (invalid: 0).
 * label_img (u8 per pixel) is preferred; with label_img == NULL the rgba8 segmentation image is
 * decoded through the colour map.  Host pointers / device pointers respectively.  The host-pointer entry counts the valid
 * pixels itself while its copies are in flight (no read-back, no host wait; buffer lifetime as for ks_integrate_points);
 * the device-pointer entry reads the compacted count back (4 bytes, one stream synchronisation) before it enqueues the frame. */
int ks_integrate_depth(ks_ctx* ctx, const float T_G_C[7], const void* depth, int depth_fmt, const uint8_t* label_img,
                       const uint8_t* rgba_img, int width, int height, const float K[4], int freespace,
                       ks_frame_stats* stats);
int ks_integrate_depth_device(ks_ctx* ctx, const float T_G_C[7], const void* d_depth, int depth_fmt,
                              const uint8_t* d_label_img, const uint8_t* d_rgba_img, int width, int height,
                              const float K[4], int freespace, ks_frame_stats* stats);

/* Layer views (host Layer<TsdfVoxel> / Layer<SemanticVoxel> contract, block edge = voxels_per_side). */
int ks_num_blocks(ks_ctx* ctx, size_t* n);
int ks_get_block_indices(ks_ctx* ctx, int32_t* out_xyz, size_t cap, size_t* n); /* sorted (x,y,z) */
/* Blocks touched since the last call with reset=1 (Block::updated(), semantic_integrator_base.cpp:248). */
int ks_get_updated_block_indices(ks_ctx* ctx, int32_t* out_xyz, size_t cap, size_t* n, int reset);
/* tsdf_out: n * vps^3 * 12 B {f32 distance, f32 weight, u8 rgba[4]};
 * sem_out:  n * vps^3 * 92 B {u8 label, 3 pad, f32 priors[21], u8 rgba[4]} (semantic_voxel.h:14-27).
 * Either may be NULL.  Absent blocks yield default-constructed voxels. */
int ks_download_blocks(ks_ctx* ctx, const int32_t* idx_xyz, size_t n, void* tsdf_out, void* sem_out);
/* Inverse of ks_download_blocks: seed / overwrite n host-layout blocks in the GPU map (same record
 * layouts; either array may be NULL to leave that half untouched).  This is how a map the host
 * already holds — the layers handed to the integrator constructor
 * (semantic_integrator_base.cpp:92-96, filled e.g. by TsdfServer::loadMap) — reaches the GPU.
 * Block indices must be distinct.  Errors: KS_ERR_POOL_FULL, KS_ERR_INDEX_RANGE. */
int ks_upload_blocks(ks_ctx* ctx, const int32_t* idx_xyz, size_t n, const void* tsdf_in, const void* sem_in);
/* Voxel-level sync for the strict drop-in mode (host Layers current after every integratePointCloud, the
 * contract behind Block::updated(), semantic_integrator_base.cpp:248): only the voxels the integrator has
 * written since the previous call travel, as KS_VOXEL_RECORD_BYTES-byte records
 *   { int32 block_x, block_y, block_z; uint32 linear_index (x + vps*(y + vps*z)); TsdfVoxel 12 B; SemanticVoxel 92 B }
 * with the voxels of one 8^3 device tile contiguous (consecutive records mostly share their block).
 * ks_count_updated_voxels sizes the buffer; ks_download_updated_voxels fills it (a page-locked buffer from
 * ks_host_alloc makes the copy run at link rate) and clears the marks.  Voxels merged in by ks_merge_tiles_device /
 * ks_reduce are reported too; voxels written by ks_upload_blocks are not (the host has them).
 * The voxel-level sync and the block-level sync (ks_get_updated_block_indices) share the per-tile "updated" flag:
 * a host uses ONE of the two (either call consumes the flag the other one reads). */
#define KS_VOXEL_RECORD_BYTES 120
/* The records of one device tile form a run that lies inside ONE host block: with the run list the host
 * finds its blocks without reading the records (runs may be NULL). */
typedef struct ks_voxel_run {
  int32_t block[3];
  uint32_t first; /* index of the run's first record */
  uint32_t count;
} ks_voxel_run;
int ks_count_updated_voxels(ks_ctx* ctx, size_t* n_records, size_t* n_runs /* may be NULL */);
int ks_download_updated_voxels(ks_ctx* ctx, void* out, size_t cap_records, size_t* n_records, ks_voxel_run* runs,
                               size_t cap_runs, size_t* n_runs);
/* Page-locked host memory for the buffers handed to ks_download_blocks / ks_upload_blocks /
 * ks_integrate_points (transfers from pageable memory go through a staging copy and run at a
 * fraction of the link rate).  ks_host_alloc returns NULL on failure. */
void* ks_host_alloc(size_t bytes);
void ks_host_free(void* p);

/* ---- semantic mesh on the device (new: the reference meshes the host layers with Voxblox's MeshIntegrator after a layer
 * sync, kimera_semantics_rosbag.cpp:147-167; here the mesh is made where the voxels are and only triangles travel) ----
 * Marching cubes over the resident tiles; the contract is DESIGN.md, section "Semantic mesh" (no parity with Voxblox's
 * mesher is claimed: it is not part of the reference tree).  In short: a cube belongs to the voxel at its lowest corner
 * and to that voxel's host-layout block (border cubes read the +x / +y / +z neighbours); it is meshed iff all eight
 * corners have weight >= min_weight; a corner is inside iff distance < 0; vertices lie on the edges between voxel CENTRES,
 * t = da / (da - db) from the lower-numbered corner; three vertices per triangle, no sharing; the normal (repeated for
 * the three vertices) points towards positive distance; a triangle of zero area is dropped and counted.  Every vertex
 * carries the colour (TsdfVoxel colour, as the context's color_mode wrote it) and the arg-max LABEL of the voxel whose
 * cell contains it.  ORDER (part of the ABI): blocks ascending by (x, y, z) like ks_get_block_indices; inside a block
 * cubes by x + vps * (y + vps * z); inside a cube triangles in table order.  Two calls on the same map give the same bytes.
 * ks_mesh_update   extracts (only_stale = 0) or refreshes (only_stale = 1) the mesh the context keeps on the device.  A
 *                  refresh re-meshes the blocks with a tile written since the last update (integrate, upload, merge, reduce,
 *                  round, reset — a per-tile flag of its own, independent of both host syncs) and the up to seven blocks at
 *                  -x / -y / -z offsets whose border cubes read them; after any sequence of calls the stored mesh is bit
 *                  for bit what a from-scratch extraction gives.  The first call, and a call with another min_weight than
 *                  the stored mesh was made with, mesh everything.  Completes the frames in flight first.
 *                  stats: blocks_meshed of blocks_total, triangles_total in the mesh, triangles_changed = triangles in the
 *                  re-meshed blocks' new segments, degenerate_dropped by this call.
 * ks_mesh_size / ks_mesh_download   the stored mesh: blocks with n_vertices > 0 in order, their segments back to back
 *                  (first_vertex / n_vertices index the four vertex arrays; xyz and normals 3 floats, rgba 4 bytes, labels
 *                  1 byte per vertex; any of the four may be NULL).  Page-locked buffers (ks_host_alloc) copy at link rate.
 * ks_mesh_changed_blocks   the blocks whose segment the LAST ks_mesh_update replaced (including ones that are empty now).
 * ks_clear / ks_clear_voxels empty the mesh too.  Errors: KS_ERR_INVALID_ARG (capacity too small; min_weight not a finite
 * positive number), KS_ERR_HIP, KS_ERR_UNSUPPORTED (a marcher context of ks_integrate_round_exact holds no voxel data).
 * Multi-GPU: each context meshes the tiles it holds; seams between the tiles of different owners are not handled. */
typedef struct ks_mesh_config { float min_weight; int32_t only_stale; } ks_mesh_config;
typedef struct ks_mesh_stats {
  uint64_t blocks_meshed, blocks_total, triangles_total, triangles_changed, degenerate_dropped;
} ks_mesh_stats;
typedef struct ks_mesh_block { int32_t block[3]; uint32_t first_vertex, n_vertices; } ks_mesh_block;
int ks_mesh_default_config(ks_mesh_config* cfg); /* min_weight 1e-4, only_stale 0 */
int ks_mesh_update(ks_ctx* ctx, const ks_mesh_config* cfg, ks_mesh_stats* stats /* may be NULL */);
int ks_mesh_size(ks_ctx* ctx, size_t* n_blocks, size_t* n_vertices);
int ks_mesh_download(ks_ctx* ctx, ks_mesh_block* blocks, size_t cap_blocks, float* xyz, float* normals, uint8_t* rgba,
                     uint8_t* labels, size_t cap_vertices);
int ks_mesh_changed_blocks(ks_ctx* ctx, int32_t* out_xyz, size_t cap, size_t* n);

/* ---- batch ESDF with nearest-surface labels on the device (new: the reference's offline program ends with
 * EsdfServer::updateEsdfBatch on the host layers, kimera_semantics_rosbag.cpp:147-167; here the distances are made where
 * the voxels are) ----
 * The contract is DESIGN.md, section "ESDF" (no parity with Voxblox's EsdfIntegrator is claimed: it is not part of the
 * reference tree and its result depends on queue order).  In short, with R = (int)ceilf(max_distance_m / voxel_size) <= 255:
 * a voxel of a resident tile with weight >= min_weight is OBSERVED; an observed voxel with |distance| < min_distance_m is a
 * SITE (Voxblox's fixed band) and keeps its TSDF distance and its own arg-max label.  Every other observed voxel v takes the
 * minimum, over the sites u of v's sign (distance < 0: negative) with |u - v| <= R on every axis in voxel indices, of the
 * key  d2 << 40 | bits(|distance_u|) << 8 | label_u  (d2 = squared index distance): the nearest site by centre distance,
 * ties to the smaller |distance|, then to the smaller label.  Its distance is
 * sign * fminf(max_distance_m, voxel_size * sqrtf((float)d2) + |distance_u|) (one multiply, one add, no contraction) and its
 * nearest label label_u; without such a site sign * max_distance_m and label 255.  Anything else is {0.0f, flags 0, label
 * 255}.  flags = observed | fixed << 1.  A label of 255 in the map (never updated) shows as 0, as in ks_download_blocks.
 * ks_esdf_update   computes the ESDF of the map as it is after the frames in flight have completed and stores it beside the
 *                  tiles (8 bytes per voxel).  Later integrate calls do not change the stored ESDF by themselves, and tiles
 *                  that join the map read as default records, until ks_esdf_refresh (below) brings it up to date;
 *                  ks_clear / ks_clear_voxels drop it.  The work space is a dense box of
 *                  voxels, the bounding box of the resident tiles (32 bytes per voxel plus 4 per tile); when it exceeds
 *                  max_workspace_bytes the call returns KS_ERR_UNSUPPORTED with stats->workspace_bytes and
 *                  stats->box_voxels filled in.  With use_region only the voxels of the host-layout blocks region_min ..
 *                  region_max (inclusive) get results — every other voxel holds a default record — and the box is the
 *                  region's tiles dilated by ceil(R / 8) tiles, clipped to that bounding box: sites outside the region
 *                  still count.  stats: voxels_observed / voxels_fixed among the voxels that got results, voxels_clamped =
 *                  observed voxels outside the band whose |distance| is max_distance_m.
 * ks_esdf_refresh  brings the stored ESDF up to date: afterwards it is, byte for byte and for every voxel of every resident
 *                  tile, what ks_esdf_update would store now with the configuration (min_weight, the two distances,
 *                  use_region and the region) of the update that made it — the refresh takes no ESDF parameters and so cannot
 *                  disagree with the store.  Every write to a tile's voxels (integrate, shard apply, upload, merge, reset)
 *                  marks the tile stale for the ESDF; the mark is a bit of its own, so the mesher (only_stale) and the two host
 *                  syncs neither consume it nor are consumed by it.  With g = ceil(R / 8), S = the resident tiles marked
 *                  stale and A = the resident tiles (inside the stored region, if any) whose tile index differs from one of
 *                  S by at most g on every axis: whole tiles of A are recomputed and nothing else is written (sufficient
 *                  because |u - v| <= R in voxels puts the tiles of u and v within floor((R + 7) / 8) = g; a record that did
 *                  not need it comes out with the same bytes).  Sites are read from every resident tile within 2 g of S.
 *                  A successful ks_esdf_update or ks_esdf_refresh clears the marks of all resident tiles; a call that fails,
 *                  a refusal for work space included, clears none and leaves the store as it was.  Work space: 8 KiB per
 *                  listed tile position of passes x and y (A dilated by g along z, and along y and z, less the positions
 *                  that can hold no key) plus 8 bytes per listed position and 4 per tile of A — it follows the stale tiles,
 *                  never a bounding box, and there is no fallback to the dense path: beyond max_workspace_bytes (0: that of
 *                  the stored update) the call returns KS_ERR_UNSUPPORTED with the stats filled in.  stats: tiles_stale = |S|,
 *                  tiles_recomputed = |A|, tiles_total = resident tiles; the three voxel counts describe the whole stored
 *                  ESDF after the call and equal what a from-scratch ks_esdf_update would report.  With nothing stale
 *                  nothing is launched over the map.  Errors: KS_ERR_INVALID_ARG (no stored ESDF), KS_ERR_UNSUPPORTED (work
 *                  space; a marcher context), KS_ERR_HIP (as in ks_esdf_update: no ESDF is stored afterwards).
 * ks_esdf_changed_blocks   the host-layout blocks that hold a tile the LAST ks_esdf_refresh recomputed, ascending by
 *                  (x, y, z) like ks_get_block_indices; empty after a ks_esdf_update until the next refresh.
 * ks_esdf_download_blocks   records of n host-layout blocks, vps^3 each in x + vps * (y + vps * z) order.
 * ks_esdf_query    the record of the voxel that contains each point (the point-to-voxel rule of the integrator for a ray's
 *                  end point); no interpolation.
 * Errors: KS_ERR_INVALID_ARG (a parameter that is not a finite positive number, R > 255, region_min > region_max, download
 * or query before any update), KS_ERR_UNSUPPORTED (work space; a marcher context of ks_integrate_round_exact), KS_ERR_HIP.
 * Multi-GPU: each context computes over the tiles it holds; seams between the tiles of different owners are not handled. */
typedef struct ks_esdf_config {
  float min_weight, min_distance_m, max_distance_m;
  int32_t use_region;
  int32_t region_min[3], region_max[3];
  uint64_t max_workspace_bytes;
} ks_esdf_config;
typedef struct ks_esdf_stats { uint64_t voxels_observed, voxels_fixed, voxels_clamped, box_voxels[3], workspace_bytes; } ks_esdf_stats;
#define KS_ESDF_RECORD_BYTES 8 /* { f32 distance; u8 flags; u8 nearest_label; u8 pad[2] } */
int ks_esdf_default_config(ks_esdf_config* cfg); /* 1e-6, 0.2 m, 2.0 m, no region, 8 GiB */
int ks_esdf_update(ks_ctx* ctx, const ks_esdf_config* cfg, ks_esdf_stats* stats /* may be NULL */);
typedef struct ks_esdf_refresh_stats {
  uint64_t tiles_stale, tiles_recomputed, tiles_total;
  uint64_t voxels_observed, voxels_fixed, voxels_clamped; /* of the whole stored ESDF after the call */
  uint64_t workspace_bytes;
} ks_esdf_refresh_stats; /* 56 bytes */
int ks_esdf_refresh(ks_ctx* ctx, uint64_t max_workspace_bytes /* 0: the stored update's */, ks_esdf_refresh_stats* stats /* may be NULL */);
int ks_esdf_changed_blocks(ks_ctx* ctx, int32_t* out_xyz, size_t cap, size_t* n);
int ks_esdf_download_blocks(ks_ctx* ctx, const int32_t* idx_xyz, size_t n, void* out /* n * vps^3 * 8 B, host block layout */);
int ks_esdf_query(ks_ctx* ctx, const float* xyz /* host, world frame */, size_t n, float* distance, uint8_t* flags,
                  uint8_t* label /* any may be NULL */);

/* ---- reads of the stored ESDF for a planner: trilinear samples with gradients, slice images, segments swept against a robot
 * radius (new: the reference sets slice_level in every launch file and hands the ESDF layer to Voxblox's planners on the host;
 * here the field is read where its records are) ----
 * The contract is DESIGN.md, section "ESDF reads"; every operation is f32 in the order written there (no parity with Voxblox's
 * interpolator is claimed: it is not part of the reference tree).  The STORE is what ks_esdf_query reads, as it is — nothing is
 * refreshed: the record of a voxel whose coordinates lie inside the packed range and whose tile was resident when the store was
 * made, otherwise the default record {0, flags 0, label 255}; tiles written since the last update or refresh hold what that call
 * stored, tiles that joined later read as default records, and after ks_remove_blocks* the store has followed the moved tiles.
 * A voxel is OBSERVED iff bit 0 of its flags is set.
 * SAMPLE E(p): g = p * voxel_size_inv - 0.5, i = floorf(g), f = g - i per axis (as the renderer's S(p)); corner j is
 * i + (j & 1, (j >> 1) & 1, j >> 2); n = the voxel ks_esdf_query takes for p.  status 0 (UNKNOWN) if a coordinate of p is not
 * finite or one of i, i + 1 is not inside the packed range (|.| < 2^20 - 1).  Otherwise status 2 (INTERPOLATED) iff all eight
 * corners are OBSERVED: distance = the interpolant of the corner distances along x, then y, then z, each step a + f * (b - a);
 * gradient_x = lerp(lerp(d1 - d0, d3 - d2, fy), lerp(d5 - d4, d7 - d6, fy), fz) * voxel_size_inv, y and z alike (the analytic
 * gradient of the interpolant, as ks_align_points takes it).  Else status 1 (NEAREST) iff n is OBSERVED: distance = that of n's
 * record, gradient 0.  Else status 0: distance = the quiet NaN 0x7fc00000, gradient 0, label 255, flags 0.  In statuses 1 and
 * 2 label and flags are those of n's record (nearest-surface label; observed | fixed << 1).
 * ks_esdf_sample   E at n host points; any of the five outputs may be NULL, not all.  Completes the frames in flight first and
 *                  stages large n in chunks.  n = 0 is no error.
 * ks_esdf_slice    an image: pixel (i, j), index j * width + i, is E at (origin + (float)i * du) + (float)j * dv per axis.  A
 *                  horizontal slice at height z: origin = (x0, y0, z), du = (voxel_size, 0, 0), dv = (0, voxel_size, 0).
 * ks_esdf_sweep    n segments {a, b} against a sphere of radius_m: d = b - a, L = sqrtf((dx dx + dy dy) + dz dz).  INVALID if a
 *                  coordinate or L is not finite or L > (float)(max_samples - 2) * min_step (min_step = min_step_m, or half the
 *                  voxel size when that is 0): t_stop 0, min_clearance +inf, t_min 0.  Otherwise u = d / L (0 when L == 0),
 *                  t = 0, and at most max_samples times: (st, dist) = E(a + t * u); st == 0 and !unknown_is_free: UNKNOWN at
 *                  t_stop = t; st != 0: c = dist - radius_m, a c below min_clearance replaces it (t_min = t), c < 0: COLLISION
 *                  at t_stop = t; then t >= L: FREE with t_stop = L; else t = fminf(t + (st != 0 ? fmaxf(c, min_step) :
 *                  min_step), L).  A segment still walking after max_samples samples is INVALID (rounding alone can do that).
 *                  Non-finite points and segments are data, not errors.
 * The *_device calls take DEVICE pointers, read and written on ks_stream(ctx): enqueued after the frames in flight have
 * completed; the host waits for the kernel only when stats is non-NULL.  The statistics are integer sums.  Two calls on the same
 * store give the same bytes.  The calls only READ: the map, the `updated` and `dirty` flags, both stale bits, the stored mesh, the
 * stored ESDF, the objects and the mesh index stay as they were.
 * Errors: KS_ERR_INVALID_ARG (NULL ctx; NULL input with n > 0; every output NULL (with n > 0); no stored ESDF; width or height
 * outside 1..8192; a non-finite origin, du or dv; radius_m or min_step_m negative or not finite; max_samples outside 2..65536;
 * n >= 2^32 segments; a context in a failed state), KS_ERR_UNSUPPORTED (a marcher context of ks_integrate_round_exact),
 * KS_ERR_HIP. */
typedef struct ks_esdf_sample_stats { uint64_t points_interpolated, points_nearest, points_unknown; } ks_esdf_sample_stats; /* 24 bytes */
enum { KS_ESDF_UNKNOWN = 0, KS_ESDF_NEAREST = 1, KS_ESDF_INTERPOLATED = 2 };
int ks_esdf_sample(ks_ctx* ctx, const float* xyz /* host, world frame */, size_t n, float* distance, float* gradient /* 3 per point */,
                   uint8_t* status, uint8_t* label, uint8_t* flags /* any may be NULL, not all */, ks_esdf_sample_stats* stats /* may be NULL */);
int ks_esdf_sample_device(ks_ctx* ctx, const float* d_xyz, size_t n, float* d_distance, float* d_gradient, uint8_t* d_status,
                          uint8_t* d_label, uint8_t* d_flags, ks_esdf_sample_stats* stats);
int ks_esdf_slice(ks_ctx* ctx, const float origin[3], const float du[3], const float dv[3], int width, int height, float* distance,
                  float* gradient, uint8_t* status, uint8_t* label, uint8_t* flags, ks_esdf_sample_stats* stats);
int ks_esdf_slice_device(ks_ctx* ctx, const float origin[3], const float du[3], const float dv[3], int width, int height,
                         float* d_distance, float* d_gradient, uint8_t* d_status, uint8_t* d_label, uint8_t* d_flags,
                         ks_esdf_sample_stats* stats);
typedef struct ks_esdf_sweep_config {
  float radius_m;          /* 0.3; >= 0 */
  float min_step_m;        /* 0: half the context's voxel_size */
  int32_t unknown_is_free; /* 0 */
  int32_t max_samples;     /* 4096; 2..65536 */
} ks_esdf_sweep_config;   /* 16 bytes */
typedef struct ks_esdf_sweep_stats {
  uint64_t segments_free, segments_collision, segments_unknown, segments_invalid, samples;
} ks_esdf_sweep_stats; /* 40 bytes */
enum { KS_SWEEP_FREE = 0, KS_SWEEP_COLLISION = 1, KS_SWEEP_UNKNOWN = 2, KS_SWEEP_INVALID = 3 };
int ks_esdf_sweep_default_config(ks_esdf_sweep_config* cfg);
int ks_esdf_sweep(ks_ctx* ctx, const float* segments /* host, n x {ax ay az bx by bz} */, size_t n, const ks_esdf_sweep_config* cfg,
                  uint8_t* status, float* t_stop, float* min_clearance, float* t_min /* any may be NULL, not all */,
                  ks_esdf_sweep_stats* stats /* may be NULL */);
int ks_esdf_sweep_device(ks_ctx* ctx, const float* d_segments, size_t n, const ks_esdf_sweep_config* cfg, uint8_t* d_status,
                         float* d_t_stop, float* d_min_clearance, float* d_t_min, ks_esdf_sweep_stats* stats);

/* ---- navigation field: cost-to-go and paths over the stored ESDF (new: the reference hands the ESDF layer to Voxblox's planners
 * on the host; here reachability, travel cost and paths are computed where the records are) ----
 * The contract is DESIGN.md, section "Navigation field".  In short: the input is the STORE the ESDF reads above describe, as it
 * is.  A voxel is TRAVERSABLE iff bit 0 of its flags is set and distance >= radius_m (an f32 compare: a NaN is not); unobserved
 * space never is (no unknown_is_free variant).  Two traversable voxels are adjacent iff their indices differ by at most 1 on every
 * axis (26-connectivity, across tile seams); a step costs KS_NAV_COST_FACE / _EDGE / _CORNER, about cost * voxel_size / 10 metres;
 * no corner-cutting rule (the radius has inflated the obstacles).  A goal's voxel is the one ks_esdf_query takes for the point; a
 * goal with a non-finite coordinate, outside the packed range or in a voxel that is not traversable counts in goals_blocked and is
 * otherwise ignored, the others (goals_used, once per point) have cost 0; all goals blocked is no error.
 * FIELD: one uint32_t per voxel of the store's tiles: KS_NAV_BLOCKED where not traversable, else the smallest sum of step costs to
 * a goal voxel, KS_NAV_UNREACHED if there is no path or that sum exceeds the cap max_cost (0: KS_NAV_MAX_COST).  It depends on the
 * store, the radius, the cap and the SET of goal voxels alone — not on slots, on the order of goals or of uploads, or on the
 * schedule of the relaxation: two calls give the same bytes.
 * ks_nav_update   completes the frames in flight (their statistics stay owed), computes the field and stores it beside the tiles
 *                 (4 B per voxel).  It only READS everything else.  The field is a SNAPSHOT of the ESDF store: later integrate,
 *                 upload, merge and fuse calls leave it, tiles that join later read KS_NAV_BLOCKED; a successful ks_esdf_update or
 *                 ks_esdf_refresh, a ks_remove_blocks* call that takes tiles out, ks_clear and ks_clear_voxels drop it, and so does
 *                 a ks_nav_update that fails.  Without a field the reads return KS_ERR_INVALID_ARG.
 * ks_nav_query    the cost of the voxel that contains each point; KS_NAV_BLOCKED outside the packed range, for non-finite points
 *                 and for tiles not in the field.
 * ks_nav_download_blocks   vps^3 words per host-layout block, x + vps * (y + vps * z); absent blocks read KS_NAV_BLOCKED.
 * ks_nav_paths    per start: v = its voxel, cost = field[v] (also when blocked or unreached).  KS_NAV_BLOCKED: PATH_BLOCKED;
 *                 unreached: PATH_UNREACHABLE; both with n_waypoints 0.  Else waypoint 0 is the centre of v,
 *                 ((float)v_k + 0.5f) * voxel_size per axis, and while field[v] > 0 the next waypoint is the FIRST neighbour u in
 *                 the order o = 0..26, o != 13, offset (o % 3 - 1, (o / 3) % 3 - 1, o / 9 - 1), with field[u] <= KS_NAV_MAX_COST and
 *                 field[u] + w(o) == field[v].  Cost 0: PATH_REACHED.  More than max_waypoints waypoints: PATH_TRUNCATED with
 *                 n_waypoints = max_waypoints.  No such neighbour (not on a field this library made): PATH_INVALID with the
 *                 waypoints so far; never looped on.  waypoints is [n][max_waypoints][3]; rows from n_waypoints on are not
 *                 written.  Any output may be NULL, not all.
 * The *_device calls take DEVICE pointers on ks_stream(ctx); the host waits only when stats is non-NULL (ks_nav_query_device has
 * none and never waits).  The host-pointer reads complete the frames in flight and stage large n in chunks.  n = 0 is no error.
 * Errors: KS_ERR_INVALID_ARG (NULL ctx or cfg; NULL goals or n_goals outside 1..65536; radius_m negative or not finite; max_cost
 * above KS_NAV_MAX_COST; max_waypoints outside 1..65536; NULL input with n > 0; every output NULL with n > 0; no stored ESDF, or
 * no stored field; a context in a failed state), KS_ERR_UNSUPPORTED (a marcher context of ks_integrate_round_exact; the
 * relaxation still active after max_rounds rounds: nothing is stored), KS_ERR_HIP. */
#define KS_NAV_BLOCKED 0xffffffffu
#define KS_NAV_UNREACHED 0xfffffffeu
#define KS_NAV_MAX_COST 0xffffff00u
enum { KS_NAV_COST_FACE = 10, KS_NAV_COST_EDGE = 14, KS_NAV_COST_CORNER = 17 };
enum { KS_NAV_PATH_REACHED = 0, KS_NAV_PATH_UNREACHABLE = 1, KS_NAV_PATH_BLOCKED = 2, KS_NAV_PATH_TRUNCATED = 3, KS_NAV_PATH_INVALID = 4 };
typedef struct ks_nav_config {
  float radius_m;      /* 0.3; >= 0, finite */
  uint32_t max_cost;   /* 0: KS_NAV_MAX_COST */
  uint32_t max_rounds; /* 0: 1 << 20 */
  uint32_t pad;
} ks_nav_config;       /* 16 bytes */
typedef struct ks_nav_stats {
  uint64_t voxels_traversable, voxels_reached, goals_used, goals_blocked, largest_cost; /* follow from the contract */
  uint64_t rounds, tile_relaxations; /* diagnostics of the schedule: they may differ from run to run */
  uint64_t workspace_bytes;          /* the field, two lists and a flag word per tile, the goals */
} ks_nav_stats;        /* 64 bytes */
typedef struct ks_nav_path_stats { uint64_t paths_reached, paths_unreachable, paths_blocked, paths_truncated, waypoints; } ks_nav_path_stats; /* 40 bytes */
int ks_nav_default_config(ks_nav_config* cfg);
int ks_nav_update(ks_ctx* ctx, const float* goals_xyz /* host, world frame */, size_t n_goals, const ks_nav_config* cfg,
                  ks_nav_stats* stats /* may be NULL */);
int ks_nav_query(ks_ctx* ctx, const float* xyz /* host, world frame */, size_t n, uint32_t* cost);
int ks_nav_query_device(ks_ctx* ctx, const float* d_xyz, size_t n, uint32_t* d_cost);
int ks_nav_download_blocks(ks_ctx* ctx, const int32_t* idx_xyz, size_t n, uint32_t* out /* n * vps^3, host block layout */);
int ks_nav_paths(ks_ctx* ctx, const float* starts_xyz /* host, world frame */, size_t n, uint32_t max_waypoints, uint8_t* status,
                 uint32_t* cost, uint32_t* n_waypoints, float* waypoints /* any may be NULL, not all */,
                 ks_nav_path_stats* stats /* may be NULL */);
int ks_nav_paths_device(ks_ctx* ctx, const float* d_starts_xyz, size_t n, uint32_t max_waypoints, uint8_t* d_status, uint32_t* d_cost,
                        uint32_t* d_n_waypoints, float* d_waypoints, ks_nav_path_stats* stats);

/* ---- view rendering: what the map looks like from a camera pose (new: the reference has no such product; a caller of it
 * downloads the layers and ray-casts on the host) ----
 * The contract is DESIGN.md, section "View rendering"; every operation is f32 in the order written there.  In short, for
 * pixel (u, v) of a width x height image, index v * width + u, with constant_x = (float)(1.0 / (double)fx) (the f32 format of
 * ks_integrate_depth), constant_y alike: dc = (((float)u - cx) * constant_x, ((float)v - cy) * constant_y, 1), uc = dc / |dc|,
 * dg = uc rotated by T_G_C, o = its translation, p(r) = o + r * dg.
 * SAMPLE S(p): g = p * voxel_size_inv - 0.5, i = floorf(g), f = g - i per axis; the eight voxels i + {0, 1}; VALID if every
 * corner index lies inside the packed range (|index| < 2^20 - 1, as ks_esdf_query), in a resident tile, with weight >=
 * min_weight; the value interpolates the distances along x, then y, then z, each step a + f * (b - a).
 * MARCH: r = min_range_m; while r <= max_range_m: s = S(p(r)); a valid s <= 0 right after a valid s_prev > 0 (at r_prev) is a
 * HIT at r_hit = r_prev + (r - r_prev) * (s_prev / (s_prev - s)); otherwise r += (valid and s > 0) ? fmaxf(s, voxel_size) :
 * voxel_size.  A NaN distance counts as invalid.  A ray that starts behind a surface, or leaves one, reports nothing there.
 * AT A HIT, p_hit = p(r_hit): depth = r_hit * uc.z (z-depth in the camera frame, what ks_integrate_depth takes); label and
 * rgba = dword 3 and dword 2 of the record of the voxel whose cell contains p_hit (floorf(p * voxel_size_inv + 1e-6), as
 * ks_esdf_query; a label of 255 shows as 0; both 0 if that tile is not resident); normal (world frame) = g / |g| with
 * g_k = S(p_hit + h e_k) - S(p_hit - h e_k), h = voxel_size, |g|^2 = (gx gx + gy gy) + gz gz — (0, 0, 0) if one of the six
 * samples is invalid or |g|^2 is not > 0; it points towards positive distance.
 * A MISS: depth = NaN, label = 255, rgba = 0, normal = 0 — the depth image can go straight back to ks_integrate_depth, which
 * drops non-finite pixels.  stats: pixels_hit + pixels_missed = width * height; samples = march samples over all pixels (an
 * integer sum).  Two calls on the same map give the same bytes.  Rendering only READS the map: the `updated` and `dirty`
 * flags, both stale bits, the stored mesh and the stored ESDF stay as they were.
 * ks_render_view          host outputs (any of the four may be NULL, not all); completes the frames in flight first.
 * ks_render_view_device   the same into DEVICE buffers, enqueued on ks_stream(ctx) after the frames in flight have completed;
 *                         the host waits for the kernel only when stats is non-NULL.
 * Errors: KS_ERR_INVALID_ARG (width or height outside 1..8192; a non-finite K, fx or fy not positive; min_weight, min_range_m
 * or max_range_m not a finite positive number; min_range_m >= max_range_m; max_range_m / voxel_size > 4096; all four outputs
 * NULL), KS_ERR_UNSUPPORTED (a marcher context of ks_integrate_round_exact), KS_ERR_HIP.  An empty map is no error: every
 * pixel misses.  Multi-GPU: each context renders the tiles it holds; a ray sees nothing of the tiles of other owners. */
typedef struct ks_render_config { float min_weight, min_range_m, max_range_m; } ks_render_config;
typedef struct ks_render_stats { uint64_t pixels_hit, pixels_missed, samples; } ks_render_stats;
int ks_render_default_config(ks_render_config* cfg); /* 1e-4, 0.1 m, 10 m */
int ks_render_view(ks_ctx* ctx, const float T_G_C[7], const float K[4] /* fx, fy, cx, cy */, int width, int height,
                   const ks_render_config* cfg, float* depth, uint8_t* labels, uint8_t* rgba /* 4 per pixel */,
                   float* normals /* 3 per pixel */, ks_render_stats* stats /* may be NULL */);
int ks_render_view_device(ks_ctx* ctx, const float T_G_C[7], const float K[4], int width, int height, const ks_render_config* cfg,
                          float* d_depth, uint8_t* d_labels, uint8_t* d_rgba, float* d_normals, ks_render_stats* stats);

/* ---- scan alignment: refine the pose of a point cloud against the resident TSDF (new: the reference's launch files select
 * Voxblox's ICP, which reads the host layer; this reads the device-resident map and needs no layer sync) ----
 * The contract is DESIGN.md, section "Scan alignment".  A Gauss-Newton alignment of the cloud to the zero level set of the
 * TSDF: point i is used iff i % point_stride == 0 and it is finite; p = T * p_C, s and its gradient from the eight corners of the
 * renderer's trilinear sample S(p) (the same validity rule); an inlier has a valid sample, |s| < max_residual_m and a non-zero
 * gradient; residual s, Jacobian row (a x grad, grad) with a = p - t: rotation about the sensor origin in the world frame, then
 * translation.  29 sums in f64 in a fixed order (no floating-point atomics), a damped 6 x 6 LDL^T solve, dq = (1, omega / 2)
 * applied from the left and renormalised, t + v; the whole loop runs on the device with one read-back at its end.
 * T_G_C_out is the last accepted pose (T_G_C_in bit for bit when no step was taken).  A status other than CONVERGED is no error.
 * stats.iterations = pose updates applied; rmse = sqrt(sum r^2 / inliers), 0 without inliers.  Two calls give the same bytes.
 * Aligning only READS the map: the `updated` and `dirty` flags, both stale bits, the stored mesh and the stored ESDF stay as
 * they were.
 * ks_align_points          xyz on the host (camera frame); completes the frames in flight first.
 * ks_align_points_device   the same with xyz a DEVICE pointer, read on the stream ks_stream returns.
 * Errors: KS_ERR_INVALID_ARG (a NULL pose or config; a non-finite pose or a zero quaternion; min_weight not a finite positive
 * number; max_residual_m, damping or an eps negative or not finite; max_iterations outside 1..64; point_stride or min_inliers
 * below 1; dof_mask 0 or above 0x3f; n >= 2^31), KS_ERR_UNSUPPORTED (a marcher context of ks_integrate_round_exact), KS_ERR_HIP.
 * n = 0 and an empty map are no errors: TOO_FEW_INLIERS with T_G_C_out = T_G_C_in.  Multi-GPU: each context aligns against the
 * tiles it holds. */
typedef struct ks_align_config {
  float min_weight;        /* 1e-4 */
  float max_residual_m;    /* 0: the context's truncation_distance */
  float damping;           /* 1e-6: times the inlier count, added to the diagonal */
  float eps_rotation_rad;  /* 1e-4 */
  float eps_translation_m; /* 1e-4 */
  int32_t max_iterations;  /* 10, 1..64 */
  int32_t point_stride;    /* 1, >= 1 */
  int32_t min_inliers;     /* 64, >= 1 */
  uint32_t dof_mask;       /* 0x3f; bits 0-2 rotation about world x, y, z, bits 3-5 translation; 0x3c = yaw + translation
                              (Voxblox's default) */
} ks_align_config;
typedef struct ks_align_stats {
  uint32_t status, iterations;
  uint64_t points_used, inliers_first, inliers_last;
  double rmse_first, rmse_last;
} ks_align_stats; /* 48 bytes */
enum { KS_ALIGN_CONVERGED = 0, KS_ALIGN_ITERATION_LIMIT = 1, KS_ALIGN_TOO_FEW_INLIERS = 2, KS_ALIGN_DEGENERATE = 3 };
int ks_align_default_config(ks_align_config* cfg);
int ks_align_points(ks_ctx* ctx, const float T_G_C_in[7], const float* xyz /* host, camera frame */, size_t n,
                    const ks_align_config* cfg, float T_G_C_out[7], ks_align_stats* stats /* may be NULL */);
int ks_align_points_device(ks_ctx* ctx, const float T_G_C_in[7], const float* d_xyz, size_t n, const ks_align_config* cfg,
                           float T_G_C_out[7], ks_align_stats* stats);

/* ---- semantic object instances: the surface of every label clustered into connected components (new: the scene-graph work
 * downstream of this map builds its objects from exactly this, on the host, from a downloaded layer) ----
 * The contract is DESIGN.md, section "Object instances".  The global index of a voxel is 8 * tile + local per axis.  A voxel of
 * a resident tile is a SURFACE voxel iff weight >= min_weight and |distance| <= surface_distance_m (a NaN distance is none); its
 * label is dword 3 of its record (255 reads as 0, as in ks_download_blocks); it TAKES PART iff it is a surface voxel, its label
 * is < 21 and bit `label` of label_mask is set.  Two voxels that take part are adjacent iff they have the same label and their
 * global indices differ by at most 1 on every axis (26-connectivity, across tile seams; a neighbour in a tile that is not
 * resident does not exist); a COMPONENT is an equivalence class of the closure, an OBJECT a component of at least min_voxels
 * voxels.  Everything in a record is an integer (no floating-point sums, no floating-point atomics):
 * centroid_k = ((double)sum_k / n_voxels + 0.5) * voxel_size is the host's one division.
 * Order (part of the ABI): objects ascend by pack_coord3(first_voxel), i.e. by (x, y, z) of their smallest voxel.  Two calls on
 * the same map give the same bytes, and so do the same voxels uploaded in another block order (nothing depends on slots).
 * ks_objects_update   clusters the map as it is after the frames in flight have completed, and stores the records and, beside
 *                     the tiles, one uint32 per voxel: the index of its object in that list, or KS_OBJECT_NONE (the voxel takes
 *                     no part; its component is below min_voxels; its tile joined the map after the call).  Later integrate
 *                     calls do not change what is stored; ks_clear and ks_clear_voxels drop it.  stats: voxels_surface = voxels
 *                     taking part, components = before the min_voxels filter, objects, voxels_in_objects,
 *                     largest_object_voxels, workspace_bytes.  The call only READS the map: the `updated` and `dirty` flags, both
 *                     stale bits, the stored mesh and the stored ESDF stay as they were.
 * ks_objects_size / ks_objects_download   the number of records / the records (cap >= that number).
 * ks_objects_download_blocks   vps^3 ids per host-layout block in x + vps * (y + vps * z) order; absent blocks read as none.
 * ks_objects_query    the id of the voxel that contains each point (the point-to-voxel rule of ks_esdf_query); out-of-range
 *                     points and non-resident tiles read as none.
 * Errors: KS_ERR_INVALID_ARG (NULL ctx or cfg; min_weight not a finite positive number; surface_distance_m negative or not
 * finite; label_mask 0 or with a bit >= 21 set; min_voxels < 1; size, download or query before any update; capacity too small),
 * KS_ERR_UNSUPPORTED (a marcher context of ks_integrate_round_exact; a map of 2^23 tiles or more, beyond what a pool can hold: a
 * voxel's id is slot * 512 + local in 32 bits), KS_ERR_HIP (nothing stays stored afterwards).  An empty map is no error: zero
 * objects.  ks_objects_download_blocks and ks_objects_query complete the frames in flight too (as ks_esdf_query does), although
 * what they read is the store of the last update.  Multi-GPU: each context clusters the tiles it holds; seams between owners are not joined. */
typedef struct ks_objects_config {
  float min_weight;         /* 1e-4 */
  float surface_distance_m; /* 0: the context's voxel_size */
  uint32_t label_mask;      /* 0x1fffff */
  uint32_t min_voxels;      /* 8 */
} ks_objects_config;
typedef struct ks_objects_stats {
  uint64_t voxels_surface, components, objects, voxels_in_objects, largest_object_voxels, workspace_bytes;
} ks_objects_stats; /* 48 bytes */
typedef struct ks_object {
  int32_t first_voxel[3]; /* the component's smallest global voxel index in (x, y, z) order: its identity */
  uint32_t n_voxels;
  int32_t bb_min[3], bb_max[3]; /* inclusive, global voxel indices */
  int64_t sum[3];               /* sums of the voxels' global indices */
  uint32_t label, pad;          /* pad = 0 */
} ks_object; /* 72 bytes */
#define KS_OBJECT_NONE 0xffffffffu
int ks_objects_default_config(ks_objects_config* cfg);
int ks_objects_update(ks_ctx* ctx, const ks_objects_config* cfg, ks_objects_stats* stats /* may be NULL */);
int ks_objects_size(ks_ctx* ctx, size_t* n);
int ks_objects_download(ks_ctx* ctx, ks_object* out, size_t cap, size_t* n);
int ks_objects_download_blocks(ks_ctx* ctx, const int32_t* idx_xyz, size_t n, uint32_t* out /* n * vps^3 ids, host block layout */);
int ks_objects_query(ks_ctx* ctx, const float* xyz /* host, world frame */, size_t n, uint32_t* id);

/* ---- exploration frontiers over the stored ESDF: the free voxels a robot can stand in that border space nobody has observed,
 * clustered (new: every exploration planner on such a map starts from this set, computed on the host from downloaded layers) ----
 * The contract is DESIGN.md, section "Exploration frontiers"; it is this library's own.  The input is the ESDF STORE exactly as
 * ks_nav_update reads it, with nothing refreshed: a voxel is OBSERVED iff bit 0 of its flags is set; every voxel outside the
 * store's tiles (a tile that is not resident, one that joined after the store was made, indices beyond the tile range) reads the
 * default record and so is not observed; a voxel is TRAVERSABLE iff it is observed and distance >= radius_m (an f32 compare: a NaN
 * is not traversable; ks_nav_update's rule).  A traversable voxel is a FRONTIER VOXEL iff at least one of its SIX face neighbours
 * is not observed (faces only); its unknown_faces is the number of such neighbours, 1..6.  With use_bounds, a voxel whose global
 * index (8 * tile + local) lies outside the inclusive box bounds_min..bounds_max is no frontier voxel; that it is unobserved still
 * makes its neighbours frontier voxels.  Frontier voxels are adjacent iff their global indices differ by at most 1 on every axis
 * (26-connectivity, across tile seams); a COMPONENT is a class of the closure, a FRONTIER a component of at least min_voxels voxels.
 * Everything in a record is an integer; centroid_k = ((double)sum_k / n_voxels + 0.5) * voxel_size is the host's one division.
 * JOIN with the navigation field: if a field is stored when ks_frontiers_update runs (it is a snapshot of this same store),
 * nav_cost is the minimum of field[v] over the frontier's voxels with field[v] <= KS_NAV_MAX_COST and nav_voxel, among the voxels
 * attaining it, the smallest in (x, y, z) order; if no voxel has such a cost, or no field is stored (no error), nav_cost =
 * KS_NAV_UNREACHED and nav_voxel = first_voxel.  The centre of nav_voxel, ((float)v + 0.5f) * voxel_size, is a valid start for
 * ks_nav_paths.  The field is read at the call: a later ks_nav_update leaves the records as they were.
 * Order (part of the ABI): frontiers ascend by pack_coord3(first_voxel).  Two calls give the same bytes, and so do the same voxels
 * uploaded in another block order (nothing depends on slots).
 * ks_frontiers_update   completes the frames in flight (their statistics stay owed) and stores the records and, beside the store's
 *                       tiles, one uint32 per voxel: the index of its frontier, or KS_FRONTIER_NONE.  The result is a snapshot of
 *                       the ESDF store, like the navigation field: later integrate, upload, merge and fuse calls leave it; a
 *                       successful ks_esdf_update or ks_esdf_refresh, a ks_remove_blocks* call that takes tiles out, ks_clear,
 *                       ks_clear_voxels and a ks_frontiers_update that fails drop it.  It only READS: the map, the `updated` and
 *                       `dirty` flags, both stale bits, the stored mesh and its index, the ESDF, the objects and the navigation
 *                       field stay as they were.  stats: voxels_traversable (of the store, whatever the bounds), voxels_frontier,
 *                       components (before the min_voxels filter), frontiers, voxels_in_frontiers, largest_frontier_voxels,
 *                       unknown_faces (over all frontier voxels), nav_field_used (0 | 1), workspace_bytes.
 * ks_frontiers_size / ks_frontiers_download   the number of records / the records (cap >= that number).
 * ks_frontiers_download_blocks   vps^3 ids per host-layout block in x + vps * (y + vps * z) order; absent blocks read as none.
 * ks_frontiers_query    the id of the voxel that contains each point (the point-to-voxel rule of ks_esdf_query).
 * Errors: KS_ERR_INVALID_ARG (NULL ctx or cfg; radius_m negative or not finite; min_voxels < 1; use_bounds with a bounds_min above
 * its bounds_max; no stored ESDF; size, download or query without a stored result; capacity too small; NULL input or output with
 * n > 0; a context in a failed state), KS_ERR_UNSUPPORTED (a marcher context of ks_integrate_round_exact; a store of 2^23 tiles or
 * more), KS_ERR_HIP (nothing stays stored).  A store without a frontier is no error: zero records; reads with n = 0 are no error.
 * Multi-GPU: each context works over the tiles it holds; tiles of another owner read as unknown, seams between owners are not joined. */
typedef struct ks_frontier_config {
  float radius_m;       /* 0.3 */
  uint32_t min_voxels;  /* 8 */
  int32_t use_bounds;   /* 0 */
  int32_t bounds_min[3], bounds_max[3]; /* inclusive, global voxel indices; read only with use_bounds */
  uint32_t pad;
} ks_frontier_config; /* 40 bytes */
typedef struct ks_frontier_stats {
  uint64_t voxels_traversable, voxels_frontier, components, frontiers, voxels_in_frontiers, largest_frontier_voxels, unknown_faces,
      nav_field_used, workspace_bytes;
} ks_frontier_stats; /* 72 bytes */
typedef struct ks_frontier {
  int32_t first_voxel[3]; /* the frontier's smallest global voxel index in (x, y, z) order: its identity */
  uint32_t n_voxels;
  int32_t bb_min[3], bb_max[3]; /* inclusive, global voxel indices */
  int64_t sum[3];               /* sums of the voxels' global indices */
  uint32_t unknown_faces;       /* sum over its voxels: proportional to the area that borders unknown space */
  uint32_t nav_cost;            /* smallest cost-to-go of its voxels, or KS_NAV_UNREACHED */
  int32_t nav_voxel[3];         /* the smallest voxel in (x, y, z) order at that cost, or first_voxel */
  uint32_t pad;                 /* 0 */
} ks_frontier; /* 88 bytes */
#define KS_FRONTIER_NONE 0xffffffffu
int ks_frontiers_default_config(ks_frontier_config* cfg);
int ks_frontiers_update(ks_ctx* ctx, const ks_frontier_config* cfg, ks_frontier_stats* stats /* may be NULL */);
int ks_frontiers_size(ks_ctx* ctx, size_t* n);
int ks_frontiers_download(ks_ctx* ctx, ks_frontier* out, size_t cap, size_t* n);
int ks_frontiers_download_blocks(ks_ctx* ctx, const int32_t* block_idx_xyz, size_t n, uint32_t* out /* n * vps^3 ids, host block layout */);
int ks_frontiers_query(ks_ctx* ctx, const float* xyz /* host, world frame */, size_t n, uint32_t* id);

/* ---- rooms over the stored ESDF: free space cut where it gets narrow, the pieces named, every free voxel and every object
 * attached to its piece, and which pieces touch where (new: the layer the scene-graph work downstream of this map builds next
 * after the objects, on the host: connected components of a truncated ESDF, a multi-source Dijkstra, a join by hand) ----
 * The contract is DESIGN.md, section "Rooms"; it is this library's own.  The input is the ESDF STORE exactly as ks_nav_update and
 * ks_frontiers_update read it, with nothing refreshed; a voxel outside the store's tiles reads the default record.
 * A voxel is OBSERVED iff bit 0 of its flags is set, FREE iff it is observed, distance >= free_distance_m (an f32 compare: a NaN is
 * not free) and, with use_bounds, its global index lies inside the inclusive box bounds_min..bounds_max; CORE iff it is free and
 * distance >= core_distance_m.  Core voxels are adjacent iff their global indices differ by at most 1 on every axis (26-connectivity,
 * across tile seams); a COMPONENT is a class of the closure, a ROOM a component of at least min_core_voxels voxels.  Order (part of
 * the ABI): rooms ascend by pack_coord3 of their smallest core voxel.
 * GROWTH: the graph is the free voxels, 26-connected, with steps of KS_NAV_COST_FACE / _EDGE / _CORNER (the graph of the navigation
 * field with free_distance_m in the place of the radius).  cost(v) is the smallest sum of step costs from v to a core voxel of any
 * room (0 on those cores); a free voxel without such a path, or with a cost above max_cost, is UNASSIGNED.  room(v) is the smallest
 * room index among the rooms that have a core voxel at exactly cost(v) from v: the lexicographic minimum of (path cost, room of the
 * path's start) over all paths.  Core voxels of components below min_core_voxels are ordinary free voxels here.
 * Per voxel of the store's tiles two uint32 are stored: the room index (KS_ROOM_NONE where the voxel is not free or unassigned) and
 * the cost (KS_NAV_BLOCKED where not free, KS_NAV_UNREACHED where unassigned).
 * ks_room: everything is an integer; bb and sum run over the ASSIGNED voxels (cores included), centroid as for ks_object;
 * clearance_bits is the bit pattern of the largest stored distance among its core voxels (a non-negative finite f32: unsigned order
 * is numeric order) and centre_voxel the smallest core voxel in (x, y, z) order attaining it: always free, and its centre
 * ((float)v + 0.5f) * voxel_size is a valid goal for ks_nav_update.
 * LINKS: an assigned voxel v of room r is a CONTACT of the link {r, q} for every q != r such that some 26-neighbour of v is assigned
 * to q (a voxel touching two other rooms counts in two links).  n_contacts counts the contacts of both sides, clearance_bits is the
 * largest stored distance among them (half the width of the passage), door_voxel the smallest contact in (x, y, z) order attaining
 * it and door_room the room that voxel is assigned to.  Links ascend by (room_a, room_b), room_a < room_b.
 * JOIN with the objects: if ks_objects_update has a stored result when ks_rooms_update runs, object i's room is the room of the
 * minimum of (cost, room) over the voxels whose stored object id is i (in slots both stores cover) that are assigned to a room, or
 * KS_ROOM_NONE; n_objects of a room counts the objects joined to it.  The objects are read at the call: a later ks_objects_update
 * leaves the rooms as they were.  Without stored objects the list is empty (no error).
 * ks_rooms_update   completes the frames in flight (their statistics stay owed) and stores the records, the links, the room of every
 *                   object and the two per-voxel planes.  The result is a snapshot of the ESDF store with the lifetime of the frontiers:
 *                   later integrate, upload, merge and fuse calls leave it; a successful ks_esdf_update or ks_esdf_refresh, a
 *                   ks_remove_blocks* call that takes tiles out, ks_clear, ks_clear_voxels and a ks_rooms_update that fails drop it.
 *                   It only READS: the map, the flags, both stale bits, the mesh and its index, the ESDF, the objects, the
 *                   navigation field and the frontiers stay as they were.  Two calls give the same bytes, and so do the same voxels
 *                   uploaded in another block order.  stats: rounds and tile_relaxations are diagnostics that may differ from run
 *                   to run; every other field is contractual (workspace_bytes: DESIGN.md §25.2).
 * ks_rooms_size / ks_rooms_download / ks_rooms_links_download   the numbers of records and links / the records / the links.
 * ks_rooms_objects  the room index per object of the join (cap >= their number, *n receives it).
 * ks_rooms_download_blocks   vps^3 values per host-layout block and plane; either output may be NULL, not both; absent blocks read
 *                   KS_ROOM_NONE and KS_NAV_BLOCKED.
 * ks_rooms_query    the room of the voxel that contains each point (the point-to-voxel rule of ks_esdf_query).
 * Errors: KS_ERR_INVALID_ARG (NULL ctx or cfg; a threshold negative or not finite; core_distance_m < free_distance_m;
 * min_core_voxels < 1; max_cost above KS_NAV_MAX_COST; use_bounds with a bounds_min above its bounds_max; no stored ESDF; reads
 * without a stored result; capacity too small; NULL input or output with n > 0; a context in a failed state), KS_ERR_UNSUPPORTED (a
 * marcher context; a store of 2^23 tiles or more; a relaxation still active after max_rounds rounds: nothing stays stored),
 * KS_ERR_HIP (nothing stays stored).  A store with no room is no error: zero records, every free voxel unassigned. */
typedef struct ks_rooms_config {
  float free_distance_m;    /* 0.0 */
  float core_distance_m;    /* 0.5 */
  uint32_t min_core_voxels; /* 64 */
  uint32_t max_cost;        /* 0: KS_NAV_MAX_COST */
  uint32_t max_rounds;      /* 0: 1 << 20, for each of the two relaxations */
  int32_t use_bounds;       /* 0 */
  int32_t bounds_min[3], bounds_max[3]; /* inclusive, global voxel indices; read only with use_bounds */
} ks_rooms_config; /* 48 bytes */
typedef struct ks_rooms_stats {
  uint64_t voxels_free, voxels_core, components, rooms, voxels_assigned, voxels_unassigned, largest_room_voxels, largest_cost, links,
      contacts, objects_seen, objects_joined, rounds, tile_relaxations, workspace_bytes;
} ks_rooms_stats; /* 120 bytes */
typedef struct ks_room {
  int32_t first_voxel[3]; /* the room's smallest core voxel in (x, y, z) order: its identity */
  uint32_t n_core_voxels;
  int32_t bb_min[3], bb_max[3]; /* inclusive, over the assigned voxels (cores included) */
  int64_t sum[3];               /* index sums over the assigned voxels */
  uint32_t n_voxels;            /* assigned voxels */
  uint32_t largest_cost;        /* over its assigned voxels */
  uint32_t clearance_bits;      /* bit pattern of the largest stored distance among its core voxels */
  int32_t centre_voxel[3];      /* the smallest core voxel in (x, y, z) order attaining it */
  uint32_t n_links, n_objects;
} ks_room; /* 96 bytes */
typedef struct ks_room_link {
  uint32_t room_a, room_b;  /* a < b */
  uint32_t n_contacts;      /* contacts of both sides */
  uint32_t clearance_bits;  /* largest stored distance among the contacts: half the width of the passage */
  int32_t door_voxel[3];    /* the smallest contact in (x, y, z) order attaining it */
  uint32_t door_room;       /* the room door_voxel is assigned to */
} ks_room_link; /* 32 bytes */
#define KS_ROOM_NONE 0xffffffffu
int ks_rooms_default_config(ks_rooms_config* cfg);
int ks_rooms_update(ks_ctx* ctx, const ks_rooms_config* cfg, ks_rooms_stats* stats /* may be NULL */);
int ks_rooms_size(ks_ctx* ctx, size_t* n_rooms, size_t* n_links /* either may be NULL, not both */);
int ks_rooms_download(ks_ctx* ctx, ks_room* out, size_t cap, size_t* n);
int ks_rooms_links_download(ks_ctx* ctx, ks_room_link* out, size_t cap, size_t* n);
int ks_rooms_objects(ks_ctx* ctx, uint32_t* room_of_object, size_t cap, size_t* n);
int ks_rooms_download_blocks(ks_ctx* ctx, const int32_t* block_idx_xyz, size_t n, uint32_t* room, uint32_t* cost /* n * vps^3 each */);
int ks_rooms_query(ks_ctx* ctx, const float* xyz /* host, world frame */, size_t n, uint32_t* room);

/* ---- view information gain over the stored ESDF: how much unobserved space each of n candidate camera poses would see (new: the
 * hot loop of a next-best-view explorer, a ray caster on the host over a downloaded layer) ----
 * The contract is DESIGN.md, section "View information gain"; it is this library's own.  The input is the ESDF STORE exactly as
 * ks_nav_update reads it, with nothing refreshed; a voxel outside the store's tiles reads the default record.  A voxel is UNKNOWN
 * iff bit 0 of its flags is clear, OCCUPIED iff observed and !(distance > stop_distance_m) (a NaN distance stops a ray), FREE
 * otherwise.  One ray per pixel of a width x height pinhole image with K = {fx, fy, cx, cy}, its origin and direction by the rule of
 * ks_render_view; samples at t_k = min_range_m + (float)k * step for k = 0 .. N - 1, N = (uint32_t)floorf((max_range_m -
 * min_range_m) / step) + 1, step = step_m or the context's voxel_size; the voxel of a sample by the point-to-voxel rule of
 * ks_esdf_query.  A ray ends OPEN before a sample that is not finite or outside the packed range, and after sample N - 1; it ends
 * as a HIT at the first sample whose voxel is occupied (that sample counts).  Unknown voxels never stop a ray.
 * A record counts the DISTINCT voxels the samples of a view's rays visit, by state (a voxel ten rays cross counts once); label_voxels
 * those occupied ones whose nearest_label equals cfg.label (0 with label = 255); samples every counted sample.  flags bit 0: the
 * view is valid.  A view whose T_G_C has a non-finite component, or whose rays leave the ball of max_range_m around its origin (a
 * quaternion that is not of unit length), is data, not an error: an all-zero record.  Views are independent; two calls give the
 * same bytes, and so do the same voxels uploaded in another block order.
 * ks_view_gain          poses and records on the host.  ks_view_gain_device: DEVICE pointers, enqueued on ks_stream(ctx); the host
 *                       is waited for only when stats is not NULL.  Both complete the frames in flight (their statistics stay
 *                       owed) and only READ: nothing is stored, nothing of the context changes.  n = 0 is no error.
 * stats: views_valid, views_invalid, the sums of the seven counters over the views, workspace_bytes and views_in_lds (DESIGN.md
 * §22.2 gives the rule for both).
 * Errors: KS_ERR_INVALID_ARG (NULL ctx or cfg; NULL poses or output with n > 0; no stored ESDF; width or height outside 1..1024 or
 * width * height > 65536; K not finite or fx, fy not positive; a range or step that is negative or not finite; min_range_m >
 * max_range_m; N > 4096; label > 255; n >= 2^24; a context in a failed state), KS_ERR_UNSUPPORTED (a marcher context of
 * ks_integrate_round_exact; the work space of one view in flight exceeds max_workspace_bytes: stats->workspace_bytes says what that
 * is, nothing else is done), KS_ERR_HIP.  Multi-GPU: each context sees the tiles it holds. */
typedef struct ks_view_gain_config {
  float min_range_m;     /* 0 */
  float max_range_m;     /* 5 */
  float step_m;          /* 0: the context's voxel_size */
  float stop_distance_m; /* 0 */
  uint32_t width;        /* 32 */
  uint32_t height;       /* 24 */
  float K[4];            /* fx, fy, cx, cy: no default, the caller sets it */
  uint32_t label;        /* 255: none */
  uint32_t pad;
  uint64_t max_workspace_bytes; /* 1 GiB */
} ks_view_gain_config; /* 56 bytes */
typedef struct ks_view_gain_record {
  uint32_t unknown_voxels, free_voxels, surface_voxels, label_voxels, rays_hit, rays_open, samples, flags;
} ks_view_gain_record; /* 32 bytes */
#define KS_VIEW_GAIN_VALID 1u
typedef struct ks_view_gain_stats {
  uint64_t views_valid, views_invalid, unknown_voxels, free_voxels, surface_voxels, label_voxels, rays_hit, rays_open, samples,
      workspace_bytes, views_in_lds;
} ks_view_gain_stats; /* 88 bytes */
int ks_view_gain_default_config(ks_view_gain_config* cfg);
int ks_view_gain(ks_ctx* ctx, const float* T_G_C /* host, n x 7 */, size_t n, const ks_view_gain_config* cfg,
                 ks_view_gain_record* out /* host, n */, ks_view_gain_stats* stats /* may be NULL */);
int ks_view_gain_device(ks_ctx* ctx, const float* d_T_G_C, size_t n, const ks_view_gain_config* cfg, ks_view_gain_record* d_out,
                        ks_view_gain_stats* stats /* may be NULL */);

/* ---- path shortening: a polyline pulled taut by line of sight over the stored ESDF (new: what every consumer of ks_nav_paths
 * did on the host over downloaded waypoints, or with one ks_esdf_sweep_device call per greedy round) ----
 * The contract is DESIGN.md, section "Path shortening"; every operation is f32 in the order written there, without FMA
 * contraction.  SW(a, b) is the sweep of ks_esdf_sweep with this call's radius_m, min_step_m, unknown_is_free and max_samples;
 * L(a, b) is the length that sweep computes.  The input is n paths in the layout ks_nav_paths writes; path i is P[0 .. m - 1], m =
 * n_waypoints_in[i].  It need not come from ks_nav_paths: the call reads the ESDF store alone, as a snapshot, exactly as
 * ks_esdf_sweep does, with or without a stored navigation field.
 * Per path: KS_SHORTEN_INVALID when m == 0, m > max_waypoints or any of the 3 m coordinates is not finite: n_out = 0, length = 0,
 * min_clearance = +inf, no sweep is taken and no row is written.  Otherwise Q[0] = P[0], a = 0, length = 0, min_clearance = +inf,
 * the status KS_SHORTEN_OK, and while a < m - 1: hi = min(a + lookahead, m - 1); the candidates j in [a + 1, hi] are taken in
 * CHUNKS OF 64 FROM THE FAR END, chunk c holding max(a + 1, hi - 64 c - 63) <= j <= hi - 64 c, and EVERY candidate of a chunk is
 * swept with SW(P[a], P[j]) (it counts in sweeps, its samples in samples); the first chunk with a FREE candidate ends the search
 * and j* is the largest FREE j of that chunk (visibility is not monotone: a free far candidate beats a blocked nearer one).  No
 * chunk with a FREE candidate: j* = a + 1, the input's own segment is kept, the path becomes KS_SHORTEN_UNVERIFIED and the
 * segment counts in segments_unverified; the call never invents geometry.  Then Q[k++] = P[j*] (the same bits), length = length
 * + L(a, j*), min_clearance = min_c of SW(P[a], P[j*]) where that is smaller, a = j*.  n_out = k; Q[n_out - 1] is P[m - 1]; m ==
 * 1 gives n_out = 1 without a sweep.  lookahead = 1 with every adjacent segment free returns the input.
 * waypoints_out is [n][max_waypoints][3]; rows from n_out on are not written.  Any output may be NULL, not all.  waypoints_out
 * may be THE SAME POINTER as waypoints_in (in place); any other overlap is the caller's error and is not detected.
 * ks_path_shorten         host pointers: completes the frames in flight (their statistics stay owed) and stages chunks of paths.
 * ks_path_shorten_device  DEVICE pointers on ks_stream(ctx).  It too completes the frames in flight first, which the host waits
 *                         for (as ks_esdf_sweep_device does); the host waits for the KERNEL only when stats is non-NULL.
 * Both only READ the context.  n = 0 is no error.  stats: integer sums; waypoints_in counts the valid paths only; sweeps and
 * samples follow from the contract.
 * Errors: KS_ERR_INVALID_ARG (NULL ctx or cfg; NULL input with n > 0; every output NULL with n > 0; max_waypoints outside
 * 1..65536; lookahead outside 1..4096; radius_m or min_step_m negative or not finite; max_samples outside 2..65536; n >= 2^32; no
 * stored ESDF; a context in a failed state), KS_ERR_UNSUPPORTED (a marcher context of ks_integrate_round_exact), KS_ERR_HIP. */
enum { KS_SHORTEN_OK = 0, KS_SHORTEN_UNVERIFIED = 1, KS_SHORTEN_INVALID = 2 };
typedef struct ks_path_shorten_config {
  float radius_m;          /* 0.3 */
  float min_step_m;        /* 0: half the context's voxel_size */
  int32_t unknown_is_free; /* 0 */
  int32_t max_samples;     /* 4096; 2..65536 */
  uint32_t lookahead;      /* 64; 1..4096 */
  uint32_t pad[3];
} ks_path_shorten_config; /* 32 bytes */
typedef struct ks_path_shorten_stats {
  uint64_t paths_ok, paths_unverified, paths_invalid, waypoints_in, waypoints_out, segments_unverified, sweeps, samples;
} ks_path_shorten_stats; /* 64 bytes */
int ks_path_shorten_default_config(ks_path_shorten_config* cfg);
int ks_path_shorten(ks_ctx* ctx, const float* waypoints_in /* host, [n][max_waypoints][3] */, const uint32_t* n_waypoints_in, size_t n,
                    uint32_t max_waypoints, const ks_path_shorten_config* cfg, uint8_t* status, uint32_t* n_waypoints_out,
                    float* waypoints_out, float* length, float* min_clearance /* any may be NULL, not all */,
                    ks_path_shorten_stats* stats /* may be NULL */);
int ks_path_shorten_device(ks_ctx* ctx, const float* d_waypoints_in, const uint32_t* d_n_waypoints_in, size_t n, uint32_t max_waypoints,
                           const ks_path_shorten_config* cfg, uint8_t* d_status, uint32_t* d_n_waypoints_out, float* d_waypoints_out,
                           float* d_length, float* d_min_clearance, ks_path_shorten_stats* stats);

/* ---- multi-GPU exchange (new functionality: the reference is single-process) ----
 * The map is a set of 8^3-voxel tiles; a tile travels as its packed 63-bit key plus a raw
 * 64 KiB record block (512 voxels x 128 B).  ks_get_tile_keys lists the resident tiles in slot
 * order; ks_export_tiles_device gathers the tiles at the given slots into a DEVICE buffer
 * (n x 65536 B); ks_merge_tiles_device merges n incoming tiles (HOST keys, DEVICE payload) into
 * the resident map: weight-averaged distance/colour and summed weight (Voxblox's layer-merge
 * rule), additive class log-likelihoods, then argmax + colour.  Keys may repeat within one
 * call (tiles of the same key received from several ranks): they are folded in array order, in
 * one kernel launch, so the result is deterministic.  ks_clear empties the map. */
#define KS_TILE_BYTES 65536
int ks_get_tile_keys(ks_ctx* ctx, uint64_t* out, size_t cap, size_t* n);
int ks_export_tiles_device(ks_ctx* ctx, const uint32_t* slots, size_t n, void* d_payload);
int ks_merge_tiles_device(ks_ctx* ctx, const uint64_t* keys, size_t n, const void* d_payload);
int ks_clear(ks_ctx* ctx);
/* Empties the MAP only: frames in flight are completed first, then every tile goes; the integrator's own state — the two
 * approximate sets of `fast`, their offsets, the clear_checks_every_n_frames counter — stays as the frames so far left it.
 * This is what voxblox::TsdfServer::clear() does to the reference's integrator (nothing); integration/server.patch calls
 * it, then uploads the semantic layer that survives clear() in the reference. */
int ks_clear_voxels(ks_ctx* ctx);
/* ---- removal of blocks from the resident map (new on this side of the boundary: voxblox::TsdfServer prunes its TSDF layer after
 * every integrated cloud with Layer::removeDistantBlocks, parameter max_block_distance_from_body; without these calls that
 * empties the host layer only, the tiles stay in HBM and host and device disagree as soon as a pruned block is touched again) ----
 * The contract is DESIGN.md §16.
 * ks_remove_blocks           takes the given host-layout blocks (edge voxels_per_side) out of the map, all (vps / 8)^3 device
 *                            tiles of a block together.  A block that is not resident is ignored, and so is a repeated index;
 *                            n = 0 removes nothing.
 * ks_remove_distant_blocks   the rule of Voxblox's Layer::removeDistantBlocks as published (Voxblox is not part of the reference
 *                            tree), evaluated on the device for every resident block, in f32, in this order, no contraction:
 *                              block_size = voxel_size * (float)vps;  o_k = (float)b_k * block_size  (the block's ORIGIN, not
 *                              its centre);  d_k = o_k - center_k;  d2 = (dx * dx + dy * dy) + dz * dz;
 *                            the block is removed iff d2 > max_distance_m * max_distance_m.  A block goes iff the rule holds for
 *                            that block; tiles are never judged one by one.
 * ks_removed_blocks          the blocks the LAST removal call took out, ascending by (x, y, z) like ks_get_block_indices (out_xyz
 *                            may be NULL to ask for the count).
 * Both removal calls complete the frames in flight first; the statistics of those frames stay owed to the next integrate call
 * or ks_flush, and the integrator's own state (the two approximate sets of `fast`, their offsets, the clear-check counter, the
 * exact early-out's table) stays as the frames left it, as with ks_clear_voxels.  Afterwards a removed block is not resident for
 * any entry point: it is absent from ks_get_block_indices, ks_get_updated_block_indices and ks_get_tile_keys, reads as default
 * voxels in ks_download_blocks, reports no voxels to ks_count_updated_voxels / ks_download_updated_voxels, and the renderer and
 * the aligner see nothing there; a later integrate, upload or merge that touches it allocates fresh tiles (counted in
 * n_blocks_allocated).  The tiles that stay keep their `updated` and `dirty` flags and both stale bits.  Slot numbers change:
 * survivors move into the freed slots (what ks_get_tile_keys lists by slot is renumbered).  Freed slots are reused and
 * pool_capacity_tiles never grows because of a removal; the pool ALLOCATION itself is not shrunk — returning memory is not part of
 * these calls.
 * The stored products: ks_mesh_update(only_stale = 1) after a removal leaves the stored mesh byte for byte what a from-scratch
 * extraction gives — the removed blocks leave it, appear in ks_mesh_changed_blocks of that update, and the resident blocks whose
 * border cubes read a removed tile are re-meshed, nothing else; until that update the stored mesh is the one of the last update.
 * ks_esdf_refresh after a removal leaves the store byte for byte what ks_esdf_update would store now (the positions of the
 * removed tiles count as stale tiles: every resident tile within g tiles of one is recomputed); with no stored ESDF nothing is
 * done.  The object records stay the snapshot of the last ks_objects_update; ids travel with their tiles, and removed blocks
 * read KS_OBJECT_NONE.
 * stats: blocks_removed, tiles_removed, tiles_moved (survivors that changed slot, at most tiles_removed), tiles_resident after
 * the call, pool_capacity_tiles.
 * Errors: KS_ERR_INVALID_ARG (NULL ctx; NULL idx_xyz with n > 0; a NULL or non-finite centre; max_distance_m negative or not
 * finite; ks_removed_blocks with a capacity that is too small; a context in a failed state), KS_ERR_INDEX_RANGE (a block index
 * outside the packed range, as ks_upload_blocks reports it), KS_ERR_UNSUPPORTED (a marcher context of ks_integrate_round_exact),
 * KS_ERR_HIP.  A call that fails before the first tile moves leaves the map as it was.
 * Multi-GPU: each context removes among the tiles it holds. */
typedef struct ks_remove_stats {
  uint64_t blocks_removed, tiles_removed, tiles_moved, tiles_resident /* after */, pool_capacity_tiles;
} ks_remove_stats; /* 40 bytes */
int ks_remove_blocks(ks_ctx* ctx, const int32_t* idx_xyz, size_t n, ks_remove_stats* stats /* may be NULL */);
int ks_remove_distant_blocks(ks_ctx* ctx, const float center[3], float max_distance_m, ks_remove_stats* stats /* may be NULL */);
int ks_removed_blocks(ks_ctx* ctx, int32_t* out_xyz, size_t cap, size_t* n); /* of the LAST removal call, ascending (x,y,z) */
/* ---- fusing a submap into the resident map at a rigid pose (new on this side of the boundary: a loop closure or a ks_align_points
 * result that corrects a submap's pose, a server that receives a layer on Voxblox's tsdf_map_in and calls
 * mergeLayerAintoLayerB(layer, T, ...), any submap-based mapper) ----
 * The contract is DESIGN.md §17; no parity with Voxblox's resampleLayer is claimed (Voxblox is not part of the reference tree).
 * ks_fuse_map resamples the map of `src` under T_D_S (qw qx qy qz tx ty tz: source frame -> destination frame) into the grid of
 * `dst` and folds the result into `dst` by the rule of ks_merge_tiles_device.  Both contexts live on the same device and have
 * bit-equal voxel_size; voxels_per_side may differ.  For every destination voxel of a candidate tile: its centre
 * c_k = ((float)v_k + 0.5f) * voxel_size goes through the inverse pose (formed on the host in f64, rounded to f32) into the source
 * frame, the source is sampled there as the renderer samples it (trilinear over the eight corners; VALID iff every corner lies
 * inside the packed range, in a resident source tile, has weight >= min_weight and a distance that is not NaN); a valid voxel's
 * incoming record is {interpolated distance, interpolated weight, the colour, label (255 as 0) and 21 priors of the NEAREST corner},
 * an invalid voxel is untouched.  A destination tile exists afterwards iff it existed before or holds a touched voxel.
 * The result depends on the voxels of the two maps, T_D_S and min_weight alone — not on slot numbers, on the enumeration of
 * candidate tiles or on the chunking by max_workspace_bytes.
 * Both contexts complete their frames in flight first; the statistics of those frames stay owed, the integrators' own state stays.
 * `src` is only read.  In `dst` every tile that holds a touched voxel is flagged for both host syncs and marked stale for the mesher
 * and the ESDF: ks_mesh_update(only_stale = 1) and ks_esdf_refresh afterwards leave the bytes of a from-scratch call; object records
 * stay the snapshot they were.
 * cfg:   min_weight (1e-4), max_workspace_bytes (1 GiB): bounds the work space of exchange-format tiles; the candidate tiles are
 *        processed in `chunks` of it.
 * stats: tiles_source (resident tiles of src), tiles_candidate (destination tiles examined), tiles_touched (those that hold a
 *        touched voxel), tiles_allocated (the touched tiles that are new in dst), voxels_fused, chunks, workspace_bytes.
 * Errors: KS_ERR_INVALID_ARG (a NULL argument; dst == src; different devices; different voxel_size; a non-finite pose or a zero
 * quaternion; min_weight not a finite positive number; a context in a failed state), KS_ERR_INDEX_RANGE (a candidate tile leaves the
 * packed tile range: reported before anything is written), KS_ERR_UNSUPPORTED (a marcher context of ks_integrate_round_exact;
 * max_workspace_bytes below what one tile needs: stats->workspace_bytes says what that is and dst is unchanged), KS_ERR_POOL_FULL,
 * KS_ERR_HIP.  An empty src is no error: all counts are 0.  Multi-GPU: each context fuses the tiles it holds. */
typedef struct ks_fuse_config {
  float min_weight;
  uint32_t pad;
  uint64_t max_workspace_bytes;
} ks_fuse_config; /* 16 bytes */
typedef struct ks_fuse_stats {
  uint64_t tiles_source, tiles_candidate, tiles_touched, tiles_allocated, voxels_fused, chunks, workspace_bytes;
} ks_fuse_stats; /* 56 bytes */
int ks_fuse_default_config(ks_fuse_config* cfg);
int ks_fuse_map(ks_ctx* dst, ks_ctx* src, const float T_D_S[7], const ks_fuse_config* cfg, ks_fuse_stats* stats /* may be NULL */);

/* ---- indexed view of the stored mesh: shared vertices (new: consumers of the mesh — deformation after a loop closure, objects
 * as vertex sets, smooth shading, a PLY that is one surface — need connectivity, and had to weld positions on the host) ----
 * The contract is DESIGN.md §18.  The input is the STORED MESH exactly as ks_mesh_download presents it: C corners (three per
 * triangle) numbered 0 .. C-1 in that layout, with that block directory.  In short:
 *   identity   corners i and j are the same vertex iff their three xyz floats are bit-equal (the cubes around an edge compute
 *              the same bits: no tolerance, no quantisation);
 *   ORDER      (part of the ABI) vertices ascend by the smallest corner number that references them; indices[i] is the vertex
 *              of corner i, so indices[0] == 0, every new maximum of indices is the previous one plus one, triangle k is
 *              indices[3k .. 3k+2], and first_vertex / n_vertices of ks_mesh_download's directory address indices unchanged;
 *   position, colour, label   those of the vertex's first corner;
 *   normal     from exact integer sums: N_k = sum over the corners of the vertex of (int32) rint(n_k * 65536.0f) (half to even)
 *              of their triangles' stored normals; s = (float) N; len = sqrtf((s_x*s_x + s_y*s_y) + s_z*s_z); s / len, or
 *              (0, 0, 0) if len is 0.  Nothing depends on the order of the additions;
 *   object id  what ks_objects_query returns for the vertex position, read when the index is built; KS_OBJECT_NONE everywhere
 *              if no objects are stored (no error).
 * Two calls on the same stored mesh give the same bytes.  The index is a SNAPSHOT of the stored mesh at the call: a later
 * ks_mesh_update (successful or not), ks_clear or ks_clear_voxels drops it; ks_remove_blocks* and ks_fuse_map leave it, as they
 * leave the stored mesh, until the next ks_mesh_update.  It is not incremental: its cost follows the corners of the stored mesh,
 * not the map.  The call reads only: the map, its flags, the stored mesh, ESDF and objects stay as they were.  It completes
 * the frames in flight first (their statistics stay owed).
 * ks_mesh_index           builds the index on the device.  stats (zeroed first): corners, vertices, the most corners on one
 *                         vertex, the bytes of work space and outputs in use.  A stored mesh of no triangle is no error.
 * ks_mesh_index_size      V and C of the current index.
 * ks_mesh_index_download  per vertex xyz and normals (3 floats), rgba (4 bytes), labels (1 byte), object_ids (u32); per corner
 *                         indices (u32).  Any output may be NULL.  The block directory is the one of ks_mesh_download.
 * Errors: KS_ERR_INVALID_ARG (NULL ctx; no stored mesh; size or download without a current index; a capacity that is too small;
 * a context in a failed state), KS_ERR_UNSUPPORTED (a marcher context of ks_integrate_round_exact), KS_ERR_HIP (no index stays
 * stored). */
typedef struct ks_mesh_index_stats {
  uint64_t corners, vertices, max_corners_per_vertex, workspace_bytes;
} ks_mesh_index_stats; /* 32 bytes */
int ks_mesh_index(ks_ctx* ctx, ks_mesh_index_stats* stats /* may be NULL */);
int ks_mesh_index_size(ks_ctx* ctx, size_t* n_vertices, size_t* n_indices);
int ks_mesh_index_download(ks_ctx* ctx, float* xyz, float* normals, uint8_t* rgba, uint8_t* labels, uint32_t* object_ids,
                           size_t cap_vertices, uint32_t* indices, size_t cap_indices);
/* Resets the tiles at the given slots to the empty state (a rank that has handed tiles to their owner keeps
 * them as empty deltas). */
int ks_reset_tiles(ks_ctx* ctx, const uint32_t* slots, size_t n);
/* Owner rank of a tile: splitmix64(key) % world. */
int ks_tile_owner(uint64_t tile_key, int world);
/* The frame-sharded path's ONE exchange step, for a C/C++ host: every rank of the RCCL
 * communicator calls it after integrating its share of a batch of frames.  rccl_comm is the caller's
 * ncclComm_t (one rank per GPU; librccl is loaded on first use, KS_RCCL_LIB overrides its path).  Tiles
 * touched since the previous reduce travel to their owner rank (all peers at once: one grouped send/recv for
 * the keys, one for the raw 64 KiB records, over xGMI); the owner folds them into its map in ascending
 * source-rank order (deterministic; weight-averaged TSDF, additive class log-likelihoods, argmax + colour);
 * the sender's copies start over as empty deltas, so the call can be repeated batch after batch without
 * counting anything twice.  Afterwards rank r holds the authoritative state of the tiles it owns.
 * COLLECTIVE: every rank calls it (a rank that returns early on a local error leaves its peers waiting, as with any
 * RCCL collective).  Steady state: the dirty-tile lists are built on the device, the exchange buffers are kept and
 * only grow; the host reads the world x world count matrix and the received keys (8 bytes per tile). */
typedef struct ks_reduce_stats {
  uint64_t tiles_sent, tiles_received, tiles_local, bytes_sent;
} ks_reduce_stats;
int ks_reduce(ks_ctx* ctx, void* rccl_comm, int rank, int world, ks_reduce_stats* stats);

/* EXACT frame-sharded integration of `fast` or `merged` — one ROUND: `world` consecutive frames, frame first_frame + r marched
 * by rank r.  COLLECTIVE: every rank calls it once per round (a rank without a frame passes n = 0), rounds in frame order.
 * `marcher` casts this rank's frame against a slot numbering of its own and evaluates the state-independent half of every
 * update; each update travels to the rank that owns its voxel's tile (ks_tile_owner) as a 20-byte record; `owner` applies the
 * frames of the round in frame order.  The tiles a rank owns are then, bit for bit, what ONE context integrating all frames in
 * order holds for them (new: the reference is a single process; replaces merging per-rank maps with ks_reduce, which is a
 * different arithmetic — SURVEY.md par. 8e).  Both contexts are created with the same method and the same configuration on every
 * rank; `marcher` is used for nothing else (its map stays empty of data).  world = 1 needs no communicator.
 *   method fast    stage A, the early-out, the emission, with the approximate sets' offsets of that GLOBAL frame number (the
 *                  frames of the other ranks advance the marcher's bookkeeping like empty clouds).
 *                  record = { tile key << 9 | voxel in tile, info byte << 24 | integration position, sdf, update weight }.
 *                  Colours from the labels, pipeline_frames = 0, "mixed" order, clear_checks_every_n_frames = 1 (or the early-out
 *                  off).  origin_voxel_touched: a frame of the round updated the voxel whose index hashes to 0 (the world
 *                  origin) — the one place where the reference's approximate sets couple frames (their zero-initialised slots
 *                  "contain" hash 0), i.e. where the result may differ from the sequential one.
 *   method merged  bundling, bundle order (either ks_config.bundle_order), bundle merge, ray casting, anti-grazing and the
 *                  clearing pass depend on nothing but the frame: no empty frames are marched for the other ranks, and
 *                  origin_voxel_touched is always 0.  sdf and update weight come from the bundle's MERGED point and weight.
 *                  record = { tile key << 9 | voxel in tile, info byte << 24 | bundle number, sdf, update weight }, where the
 *                  marcher numbers the frame's bundles that have an update 0 .. B-1 (info byte: label | kind << 5 | clearing
 *                  << 7; kind 1 = pure-label, 2 = mixed-label bundle).  The semantic increments travel as the marcher computed
 *                  them, in two tables per frame that go, whole, to every peer that receives a record of the frame:
 *                    bundle table  B x 8 bytes { d_match, d_non }; a mixed-label bundle: { its row in the mixed table (u32), - }
 *                    mixed table   84 bytes (21 f32) per mixed-label bundle
 *                  Colours from the labels (KS_COLOR_MODE_COLOR blends by the voxel's weight at each update, which a record does
 *                  not carry: KS_ERR_UNSUPPORTED), pipeline_frames = 0; every integration_order_mode.  rays_cast = bundles.
 * bytes_sent counts every byte that leaves the rank: records and, for `merged`, the tables once per receiving peer.
 * A cloud of 2^24 points or more does not fit the record's 24-bit field: KS_ERR_INVALID_ARG (both methods).
 * FAILURES.  What is the same on every rank by contract (the configuration, a missing librccl) is refused before anything is
 * exchanged.  What can differ from rank to rank — a label >= 21, a cloud too large, rounds out of order, a context retired by an
 * earlier failure — is carried in the round's count exchange: no rank is left waiting, the failing rank returns its own code,
 * every other rank KS_ERR_PEER_FAILED with a text naming the rank and its code, and NO rank applies anything of the round.  A
 * `merged` marcher is put back where it was (the round can be repeated by every rank); a `fast` marcher whose per-call state has
 * already advanced cannot be, and is retired (every later call on it returns KS_ERR_INVALID_ARG).  A HIP / RCCL failure inside the
 * exchange itself cannot be told to the peers (as with ks_reduce and any RCCL collective). */
typedef struct ks_round_stats {
  uint64_t updates_marched, updates_applied, bytes_sent, origin_voxel_touched, rays_cast;
} ks_round_stats;
int ks_integrate_round_exact(ks_ctx* marcher, ks_ctx* owner, void* rccl_comm, int rank, int world, uint64_t first_frame,
                             const float T_G_C[7], const float* xyz, const uint8_t* rgba, const uint8_t* labels, size_t n,
                             int freespace_points, ks_round_stats* stats);

/* Diagnostics (used by tests): stable LSD radix sort of n HOST keys (key_bits = 32 or 64, bits
 * [0,end_bit)) and optional u32 payload with the library's own GPU sort. */
int ks_debug_radix_sort(ks_ctx* ctx, void* keys, uint32_t* vals, size_t n, int key_bits, unsigned end_bit);
/* ... of the bits [begin_bit, end_bit) only (end_bit is clamped to key_bits; an empty range leaves the arrays as they are):
 * keys that are equal in those bits keep their order, whatever their other bits hold, and every key arrives whole.  vals may be
 * NULL.  In place on the host arrays, through the context's own sorts and their persistent workspace: consecutive calls on one
 * context alternate between the workspace's halves as a context's frames do.  key_bits other than 32 / 64, or a NULL keys with
 * n > 0: KS_ERR_INVALID_ARG. */
int ks_debug_radix_sort_range(ks_ctx* ctx, void* keys, uint32_t* vals, size_t n, int key_bits, unsigned begin_bit, unsigned end_bit);
/* ... and the form whose key counts live in device memory: nb (1 .. 8) sorts of u64 keys with u32 payload in one launch sequence,
 * sort i over the first min(counts[i], cap) entries of keys[i * cap ...] / vals[i * cap ...], bits [begin_bit, end_bit) as above.
 * The sort ping-pongs between the uploaded arrays (a) and a second buffer set (b) filled with the byte 0xA5, one 8-bit pass at a
 * time; what comes back, in place, is the WHOLE buffer that holds the result, all cap entries of it: b after an odd number of
 * passes, else a.  Its entries from the count on are therefore 0xA5 bytes (b), or whatever a holds there (after two passes: the
 * input), unless the sort wrote where it must not.  No graph capture.  NULL arrays, cap = 0 or >= 2^32, an empty or reversed bit
 * range, end_bit > 64 and whatever the batched sort itself refuses (nb < 1, nb > 8): KS_ERR_INVALID_ARG. */
int ks_debug_radix_sort_batch(ks_ctx* ctx, uint64_t* keys, uint32_t* vals, const uint64_t* counts, int nb, size_t cap,
                              unsigned begin_bit, unsigned end_bit);

int ks_synchronize(ks_ctx* ctx);
void* ks_stream(ks_ctx* ctx); /* the hipStream_t that reads the caller's device inputs (stage A; with
                                * pipeline_frames the later stages run on further internal streams) */
/* Finish the frames a pipelined context still holds (no-op otherwise); stats = theirs, summed. */
int ks_flush(ks_ctx* ctx, ks_frame_stats* stats);
/* level 0: off; 1: events around every stage and every k_apply dispatch (costs ~50 us of stream
 * bubbles per frame); 2: only the k_apply dispatch of every 4th frame is timed (a few us/frame).
 * Events are resolved lazily, never by a host wait inside a frame. */
int ks_profile_enable(ks_ctx* ctx, int level);
/* Exact early-out contexts: frames integrated and fix-point rounds run so far (either may be NULL). */
int ks_early_out_iterations(ks_ctx* ctx, uint64_t* frames, uint64_t* iterations);
/* ... and out[0] = frames, out[1] = rounds, out[2] = frames that fell back to the host-driven loop (buffers that had to
 * grow, round limit), out[3] = 1 if the event-driven loop is in use, out[4] = 1 if frames are pipelined (returns KS_OK). */
int ks_early_out_stats(ks_ctx* ctx, uint64_t out[5]);
int ks_profile_get(ks_ctx* ctx, ks_profile* out, int reset);
/* The voxel update's handling of the runs of more than 1024 updates (the voxels next to the sensor) since the context was
 * created: out[0] = runs whose class sums went through the integer-sum path (csrc/ks_k_apply_xl.h), out[1] = runs the serial
 * kernel took, out[2] = 64-update chunks on the first path, out[3] = of them, replayed update by update.  Completes the frames
 * in flight first. */
int ks_update_stats(ks_ctx* ctx, uint64_t out[4]);
/* How the context pipelines: out[0] = frames of lag in effect (0: one frame at a time — what ks_create made of
 * ks_config.pipeline_frames), out[1] = frame slots, out[2] = frames per stage-B batch, out[3] = march streams. */
int ks_pipeline_shape(ks_ctx* ctx, int32_t out[4]);
/* Which chain of a frame runs on which stream.  The runtime spreads a process's streams over its hardware queues
 * and runs kernels of streams that share a queue one after the other, so ks_create fits the context's streams into the queues
 * the process has: out[0] = that budget (GPU_MAX_HW_QUEUES as the library found it — it only reads it —, 4 when unset or no
 * number, 1..32), out[1] = distinct streams the context created, out[2] = march streams (= ks_pipeline_shape's), out[3] = the
 * long-run update (k_apply_long): 1 a stream of its own beside k_apply, 0 on the stage-T stream behind it, out[4] = the same for
 * the runs of more than 1024 updates (k_apply_xlong; -1: no such kernel, KS_XLONG=0), out[5] = stage B has streams of its own
 * (0: it follows stage A on stage A's), out[6] = stage T has a stream of its own (0: unpipelined, stage A's), out[7] = streams
 * the context holds (= out[1]).  Stage A, stage B and stage T never give up a stream; the two side chains do, xlong first, while
 * the context would otherwise need more streams than the budget — below a budget of 8: from there on every context has the
 * layout it always had.  The map is the same for every plan. */
int ks_stream_plan(ks_ctx* ctx, int32_t out[8]);
/* The tail of a pipelined `fast` context.  Stage B goes out per batch of frames (ks_pipeline_shape's out[2]);
 * where every frame of a batch is one the tail would simply sort and apply, the batch's updates are sorted and applied in ONE
 * pass at the tail of its first frame — every voxel in (frame, integration position) order: the same map, the same
 * ks_frame_stats at every call.  Since the context was created: out[0] = batches applied in one pass, out[1] = frames in them,
 * out[2] = batches whose frames' tails ran one by one instead (a frame with an error, a fix point that fell back, pairs that
 * did not fit, a frame large enough for k_apply_runs, the stage profile, KS_DEBUG=1 KS_TAIL_BATCH=0), out[3] = updates applied by
 * the passes of out[0].  Batches of one frame and contexts whose pair keys carry no frame index count nowhere. */
int ks_tail_batch_stats(ks_ctx* ctx, uint64_t out[4]);
/* Diagnostics (host arithmetic, no device involved): the rule behind out[0] / out[2] above for a batch of nb frames whose
 * snapshots hold the error bits err[k] and the update counts n_pairs[k], in a context that is (not) a marcher of
 * ks_integrate_round_exact, at that profiling level, with k_apply_runs from apply_runs_min_pairs updates per frame on.
 * Returns 1 (one pass), 0 (frame by frame) or KS_ERR_INVALID_ARG. */
int ks_tail_batch_rule(const uint32_t* err, const uint64_t* n_pairs, int32_t nb, int32_t marcher, int32_t profiling, uint64_t apply_runs_min_pairs);
/* Diagnostics (host arithmetic, no device involved): the launch shape of the early-out's ordered phases for a context whose
 * frame slots hold cap_points points, integration_order_mode and early_out_phase_growth (16..4096) as in ks_config.  Per phase
 * j < max_phases: out[3 j] and out[3 j + 1] = its generations [g0, g1), out[3 j + 2] = wavefronts launched per frame = the most
 * (chain, sub-run) work items any frame of at most cap_points points can have in that phase (0: no such frame reaches the
 * phase; it is not launched).  Returns the number of phases (>= 0; out may be NULL with max_phases = 0) or KS_ERR_INVALID_ARG. */
int ks_seed_launch_shape(int32_t integration_order_mode, int32_t early_out_phase_growth, uint64_t cap_points, uint32_t* out, int32_t max_phases);

#ifdef __cplusplus
}
#endif
#endif /* KS_HIP_H_ */
