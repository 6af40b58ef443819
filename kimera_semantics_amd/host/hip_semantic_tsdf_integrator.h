// kimera::HipSemanticTsdfIntegrator — the MI355X integrator behind the reference's plugin
// surface.  Same bases, same constructor arguments and the same virtual as
//   kimera::FastSemanticTsdfIntegrator   (kimera_semantics/include/kimera_semantics/semantic_tsdf_integrator_fast.h:63-86)
//   kimera::MergedSemanticTsdfIntegrator (kimera_semantics/include/kimera_semantics/semantic_tsdf_integrator_merged.h:56-86)
// so SemanticTsdfServer (kimera_semantics_ros/src/semantic_tsdf_server.cpp:71-78) can hold it
// through std::unique_ptr<vxb::TsdfIntegratorBase> unchanged.  All integration work happens in
// libks_hip.so (include/ks_hip.h); this class only marshals arguments and keeps the host
// Layers consistent.
#pragma once
#include <condition_variable>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <voxblox/integrator/tsdf_integrator.h>

#include "kimera_types.h"
#include "ks_hip.h"

namespace kimera {

class HipSemanticTsdfIntegrator : public vxb::TsdfIntegratorBase, public SemanticIntegratorBase {
 public:
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  enum class Method : int { kFast = KS_METHOD_FAST, kMerged = KS_METHOD_MERGED };

  /// When the host Layers are refreshed from the GPU map.
  enum class SyncPolicy {
    kEveryFrame,  ///< strict drop-in: Layers are current when integratePointCloud returns
    kOnDemand     ///< call syncLayers() before meshing / saving (e.g. from the mesh timer)
  };

  struct DeviceOptions {
    int device_id = 0;
    uint32_t max_tiles = 1u << 16;   ///< 8^3-voxel tiles (49.7 KB each)
    uint32_t max_points = 1u << 20;
    SyncPolicy sync_policy = SyncPolicy::kEveryFrame;
    /// ks_config.pipeline_frames (0 .. 16; 16 = batches of eight frames, twice the frame slots): how many calls the second half of a frame may lag behind.  The context is
    /// created able to pipeline whatever the policy: under kEveryFrame every call completes its frame anyway (the layer sync
    /// does), and a server that switches to kOnDemand AFTER the factory handed the integrator out (integration/server.patch)
    /// gets overlapping frames without the integrator being rebuilt.  0: never pipeline.
    int pipeline_frames = 8;
    /// syncLayers() moves only the VOXELS written since the previous sync (ks_download_updated_voxels: 120-byte
    /// records scattered into the host blocks) instead of whole updated blocks (ks_download_blocks).
    bool voxel_sync = true;
    /// `fast` with the early-out enabled (ks_config.early_out_phase_growth): 0 = the map the reference produces at
    /// integrator_threads = 1 (its deterministic case), bit for bit — the default, whatever Config::integrator_threads
    /// says (with more threads the reference itself is racy: any of its results is within its own spread of this
    /// one); 16..4096 = the ordered-phase schedule alone (a few launches cheaper, not the reference's map).
    int early_out_phase_growth = 0;
    /// integration_order_mode "mixed": -1 (default) = the permutation probeMixedOrder() reads from the Voxblox this build
    /// links (LOG(FATAL) if it is neither known form); KS_ORDER_MIXED / KS_ORDER_MIXED_1024_GROUPS force one.
    int mixed_order = -1;
  };

  /// The permutation vxb::ThreadSafeIndexFactory::get("mixed", ...) of this build hands out: KS_ORDER_MIXED,
  /// KS_ORDER_MIXED_1024_GROUPS, -1 (neither), -2 (built against the interface-only stand-in headers: no Voxblox to ask).
  static int probeMixedOrder();

  HipSemanticTsdfIntegrator(Method method, const Config& config, const SemanticConfig& semantic_config,
                            vxb::Layer<vxb::TsdfVoxel>* tsdf_layer, vxb::Layer<SemanticVoxel>* semantic_layer,
                            const DeviceOptions& options);
  HipSemanticTsdfIntegrator(Method method, const Config& config, const SemanticConfig& semantic_config,
                            vxb::Layer<vxb::TsdfVoxel>* tsdf_layer, vxb::Layer<SemanticVoxel>* semantic_layer);
  ~HipSemanticTsdfIntegrator() override;

  /// The virtual the server calls; labels are decoded from the colours on the GPU through the
  /// colour->label table (the reference's serial host loop, fast.cpp:150-158 / merged.cpp:73-88).
  void integratePointCloud(const vxb::Transformation& T_G_C, const vxb::Pointcloud& points_C,
                           const vxb::Colors& colors, const bool freespace_points = false) override;

  /// Label-aware overload (MergedSemanticTsdfIntegrator, merged.h:82-86).
  void integratePointCloud(const vxb::Transformation& T_G_C, const vxb::Pointcloud& points_C,
                           const HashableColors& colors, const SemanticLabels& semantic_labels,
                           const bool freespace_points = false);

  /// Copies every block touched since the last call into the host Layers (allocating blocks
  /// as needed) and sets Block::updated(), as semantic_integrator_base.cpp:248 does.
  void syncLayers();
  void syncLayersByBlock();  ///< the whole-block variant (DeviceOptions::voxel_sync = false)
  /// Host layers -> GPU map (every allocated block).  Called by the constructor when the layers it
  /// is handed are not empty (a map loaded with TsdfServer::loadMap), so the integrator continues
  /// from the map the host holds exactly like the CPU integrators do.
  void uploadLayers();

  /// Switch between the strict and the on-demand policy at run time (integration/server.patch: a server that calls
  /// syncLayers() where it reads the Layers selects kOnDemand right after the factory handed the integrator out).
  void setSyncPolicy(SyncPolicy policy) { options_.sync_policy = policy; }
  /// Empties the GPU map.  keep_integrator_state: only the voxels go, the approximate sets and frame counters of `fast` stay
  /// (ks_clear_voxels) — vxb::TsdfServer::clear() removes the TSDF blocks and leaves the integrator and the semantic layer
  /// alone: integration/server.patch syncs, lets the base class clear, empties the GPU map this way and uploads what survived.
  void clearDeviceMap(bool keep_integrator_state = false);
  /// vxb::Layer::removeDistantBlocks for a map that lives on the GPU (ks_remove_distant_blocks; the contract is DESIGN.md,
  /// section 16): every block whose ORIGIN is further than max_distance from center leaves the device map, and the same blocks
  /// (ks_removed_blocks) leave the host TSDF layer, so host and device keep agreeing when a pruned block is touched again.
  /// keep_semantic_layer = true is what the reference does: vxb::TsdfServer prunes the TSDF layer it knows and the semantic
  /// blocks survive — the host layers are brought up to date first, and the surviving semantic halves go back up afterwards
  /// (ks_upload_blocks with no TSDF half: the blocks are resident again, with default TSDF voxels — the device holds a block's two
  /// halves together, so this mode frees no device memory).  false removes the host semantic blocks too: the map really shrinks.
  /// Returns the number of blocks removed.  integration/server.patch calls it where vxb::TsdfServer prunes.
  size_t removeDistantBlocks(const vxb::Point& center, vxb::FloatingPoint max_distance, bool keep_semantic_layer = true);
  const ks_remove_stats& lastRemoveStats() const { return last_remove_stats_; }
  /// A server that prunes (vxb::TsdfServer, parameter max_block_distance_from_body) hands its radius over once: from then on
  /// every integratePointCloud ends with removeDistantBlocks(T_G_C.getPosition(), max_distance, keep_semantic_layer) — right
  /// before the base class prunes its host TSDF layer, which then finds nothing left to do.  The largest FloatingPoint (the
  /// server's default) switches it off.  keep_semantic_layer = true brings the host layers up to date after every frame.
  void setMaxBlockDistanceFromBody(vxb::FloatingPoint max_distance, bool keep_semantic_layer = true) {
    prune_distance_ = max_distance;
    prune_keep_semantic_ = keep_semantic_layer;
  }

  /// One block of the semantic mesh: the fields of vxb::Mesh (three vertices per triangle, no indices) plus the arg-max
  /// label of the voxel that contains each vertex, in types this adapter already uses.
  struct MeshBlock {
    vxb::BlockIndex index;
    std::vector<vxb::Point> vertices, normals;
    std::vector<vxb::Color> colors;
    std::vector<uint8_t> labels;
  };
  /// Refreshes the mesh ON THE DEVICE (ks_mesh_update: marching cubes over the resident tiles) and hands back the blocks
  /// whose mesh it replaced — blocks that are empty now included, so a caller can clear them.  Needs NO syncLayers(): the
  /// voxels stay in HBM, only triangles travel.  only_mesh_updated_blocks = false meshes everything.  Returns true when
  /// `changed` is not empty.  What vxb::MeshIntegrator::generateMesh + the layer sync before it do in the reference's
  /// server ("Mesh without a layer sync").
  bool updateMesh(bool only_mesh_updated_blocks, std::vector<MeshBlock>* changed);
  const ks_mesh_stats& lastMeshStats() const { return last_mesh_stats_; }

  /// The mesh updateMesh() left on the device with SHARED vertices (ks_mesh_index; the contract is DESIGN.md §18): what a consumer
  /// that needs connectivity takes instead of welding positions — mesh deformation after a loop closure, objects as vertex
  /// sets, smooth shading.  Vertices ascend by the first corner that references them; triangle k is indices[3k .. 3k+2];
  /// `blocks` is the directory of the stored mesh (first_vertex / n_vertices address `indices`); object_ids are
  /// KS_OBJECT_NONE unless updateObjects() has run.
  struct IndexedMesh {
    std::vector<vxb::Point> vertices, normals;
    std::vector<vxb::Color> colors;
    std::vector<uint8_t> labels;
    std::vector<uint32_t> object_ids, indices;
    std::vector<ks_mesh_block> blocks;
    ks_mesh_index_stats stats{};
  };
  /// Builds the index of the STORED mesh on the device and fetches it.  Needs no syncLayers() and no mesh update of its own:
  /// call updateMesh() first (it throws where no mesh is stored).  Not incremental: the cost follows the triangles of the
  /// stored mesh.  Returns true when the mesh has a triangle.
  bool indexMesh(IndexedMesh* out);

  /// Batch ESDF with nearest-surface labels (ks_esdf_update; the contract is DESIGN.md, "ESDF") in this adapter's own types:
  /// there is no Voxblox EsdfVoxel behind it and no parity with vxb::EsdfIntegrator is claimed.  Defaults as
  /// vxb::EsdfIntegrator::Config.  With use_region only the blocks region_min .. region_max (inclusive) get results.
  struct EsdfOptions {
    float min_weight = 1e-6f, min_distance_m = 0.2f, max_distance_m = 2.0f;
    uint64_t max_workspace_bytes = 8ull << 30;
    bool use_region = false;
    vxb::BlockIndex region_min = vxb::BlockIndex(0, 0, 0), region_max = vxb::BlockIndex(0, 0, 0);
  };
  struct EsdfVoxel {         ///< one record of ks_esdf_download_blocks
    float distance;          ///< signed, |distance| <= max_distance_m; a site keeps its TSDF distance
    uint8_t flags;           ///< observed | fixed << 1
    uint8_t nearest_label;   ///< label of the nearest surface voxel; 255: none within reach (or not observed)
    uint8_t pad[2];
  };
  struct EsdfBlock {
    vxb::BlockIndex index;
    std::vector<EsdfVoxel> voxels;   ///< voxels_per_side^3, x + vps * (y + vps * z)
  };
  /// Computes the ESDF of the whole map ON THE DEVICE, as it is after the frames in flight, and hands back every block of
  /// the map (ascending by x, y, z).  Needs NO syncLayers().  What EsdfServer::updateEsdfBatch does at the end of the
  /// reference's offline program ("ESDF"), and the first call of a server that keeps an ESDF up to date.
  /// Returns true when `out` is not empty.
  bool updateEsdf(const EsdfOptions& options, std::vector<EsdfBlock>* out);
  const ks_esdf_stats& lastEsdfStats() const { return last_esdf_stats_; }
  /// Brings the ESDF of the last updateEsdf() up to date with the map ON THE DEVICE (ks_esdf_refresh: only the tiles that
  /// the tiles written since can reach are recomputed, with the options of that updateEsdf()) and hands back only the blocks
  /// that hold a recomputed tile, with their records (ascending by x, y, z): what the timer of an ESDF server calls.  The
  /// records of every other block are what they were.  Returns true when `changed` is not empty.
  bool refreshEsdf(std::vector<EsdfBlock>* changed);
  const ks_esdf_refresh_stats& lastEsdfRefreshStats() const { return last_esdf_refresh_stats_; }
  /// Distance and gradient of the STORED ESDF at world points (ks_esdf_sample; the contract is DESIGN.md, "ESDF reads"): the
  /// trilinear interpolant where all eight corner voxels are observed (status 2), the nearest voxel's distance with a zero
  /// gradient where only the point's own voxel is (status 1), NaN otherwise (status 0).  What a planner asked of Voxblox's
  /// EsdfMap::getDistanceAndGradientAtPosition, ON THE DEVICE: no ESDF layer travels.  The store is read as it is — call
  /// updateEsdf() / refreshEsdf() first.  Returns true when at least one point is not unknown.
  struct EsdfSamples {
    std::vector<float> distance;
    std::vector<vxb::Point> gradient;
    std::vector<uint8_t> status, label, flags;   ///< KS_ESDF_*; nearest-surface label; observed | fixed << 1
  };
  bool sampleEsdf(const vxb::Pointcloud& points_G, EsdfSamples* out);
  const ks_esdf_sample_stats& lastEsdfSampleStats() const { return last_esdf_sample_stats_; }
  /// Segments against a sphere of radius_m over the STORED ESDF (ks_esdf_sweep): how a sampling planner validates an edge.
  /// status is KS_SWEEP_FREE / COLLISION / UNKNOWN / INVALID; t_stop the arc length where the walk ended, min_clearance the
  /// smallest distance - radius seen on the way and t_min where.  Returns true when every segment is FREE.
  struct SweepOptions {
    float radius_m = 0.3f, min_step_m = 0.0f;   ///< min_step_m 0: half a voxel
    bool unknown_is_free = false;
    int max_samples = 4096;
  };
  struct EsdfSegment {
    vxb::Point a, b;
  };
  struct EsdfSweeps {
    std::vector<uint8_t> status;
    std::vector<float> t_stop, min_clearance, t_min;
  };
  bool sweepEsdf(const std::vector<EsdfSegment>& segments, const SweepOptions& options, EsdfSweeps* out);
  const ks_esdf_sweep_stats& lastEsdfSweepStats() const { return last_esdf_sweep_stats_; }
  /// The cost-to-go field of the STORED ESDF to the nearest of `goals_G`, through the voxels a sphere of radius_m may occupy
  /// (ks_nav_update; the contract is DESIGN.md, "Navigation field"): what a planner computed by Dijkstra on a downloaded ESDF
  /// layer, ON THE DEVICE.  The field stays there for planPaths() until the next updateEsdf() / refreshEsdf(), removal or clear.
  /// Call updateEsdf() / refreshEsdf() first.  Returns true when at least one goal is usable.
  struct NavOptions {
    float radius_m = 0.3f;
    uint32_t max_cost = 0;     ///< 0: KS_NAV_MAX_COST
    uint32_t max_rounds = 0;   ///< 0: 1 << 20
  };
  bool updateNavField(const vxb::Pointcloud& goals_G, const NavOptions& options);
  const ks_nav_stats& lastNavStats() const { return last_nav_stats_; }
  /// A path per start by steepest descent of that field (ks_nav_paths): waypoints are voxel centres, the last one a goal's.
  /// status is KS_NAV_PATH_*; cost the start voxel's field value (about cost * voxel_size / 10 metres when reached).
  /// Returns true when every start reached a goal.
  struct NavPaths {
    std::vector<uint8_t> status;
    std::vector<uint32_t> cost;
    std::vector<vxb::Pointcloud> waypoints;
  };
  bool planPaths(const vxb::Pointcloud& starts_G, uint32_t max_waypoints, NavPaths* out);
  const ks_nav_path_stats& lastNavPathStats() const { return last_nav_path_stats_; }
  /// Polylines pulled taut by line of sight over the STORED ESDF (ks_path_shorten; the contract is DESIGN.md, "Path shortening"):
  /// of each path only the waypoints stay from which the next kept one is reachable in a straight line with the clearance
  /// radius_m, looking at most `lookahead` waypoints ahead.  The paths need not come from planPaths(), and no navigation field
  /// is needed.  status is KS_SHORTEN_*: a segment that no sweep could verify is kept as the input has it (UNVERIFIED); an empty
  /// path, one with a non-finite coordinate or one of more than 65536 waypoints (the library's largest max_waypoints) is INVALID and
  /// comes back empty; the other paths of the call are not affected.  Returns true when every path is KS_SHORTEN_OK.
  struct ShortenOptions {
    float radius_m = 0.3f;
    float min_step_m = 0.0f;     ///< 0: half a voxel
    bool unknown_is_free = false;
    int32_t max_samples = 4096;
    uint32_t lookahead = 64;     ///< 1..4096
  };
  struct ShortPaths {
    std::vector<uint8_t> status;
    std::vector<vxb::Pointcloud> waypoints;
    std::vector<float> length, min_clearance;
  };
  bool shortenPaths(const std::vector<vxb::Pointcloud>& paths, const ShortenOptions& options, ShortPaths* out);
  const ks_path_shorten_stats& lastPathShortenStats() const { return last_path_shorten_stats_; }
  /// What the map looks like from a camera pose (ks_render_view; the contract is DESIGN.md, "View rendering"): one ray per
  /// pixel through the resident tiles ON THE DEVICE, as the map is after the frames in flight.  Needs NO syncLayers(): the
  /// voxels stay in HBM, only the images travel.  depth is z-depth in the camera frame, NaN where the ray found no surface
  /// (label 255, colour and normal 0 there); normals are in the world frame and stay empty with options.normals = false.
  struct RenderOptions {
    float min_weight = 1e-4f, min_range_m = 0.1f, max_range_m = 10.0f;
    bool normals = true;
  };
  struct RenderedView {
    int width = 0, height = 0;             ///< pixel (u, v) at v * width + u
    std::vector<float> depth;
    std::vector<uint8_t> labels;
    std::vector<vxb::Color> colors;
    std::vector<vxb::Point> normals;
  };
  /// Returns true when at least one pixel hit a surface.
  bool renderView(const vxb::Transformation& T_G_C, float fx, float fy, float cx, float cy, int width, int height,
                  const RenderOptions& options, RenderedView* out);
  const ks_render_stats& lastRenderStats() const { return last_render_stats_; }
  /// Refines the pose of a cloud against the TSDF of the map ON THE DEVICE (ks_align_points; the contract is DESIGN.md, "Scan
  /// alignment"): what Voxblox's ICP (`enable_icp`) does against the host layer, as the map is after the frames in flight.
  /// Needs NO syncLayers(): the voxels stay in HBM, only the cloud and the pose travel.  dof_mask: bits 0-2 rotation about
  /// world x, y, z, bits 3-5 translation; 0x3c = yaw and translation, Voxblox's default.  max_residual_m = 0: the truncation
  /// distance.  *T_refined is the last accepted pose (T_G_C itself when no step was taken); lastAlignStats().status says how
  /// the loop ended.  Returns true when at least one step was taken.
  struct AlignOptions {
    float min_weight = 1e-4f, max_residual_m = 0.0f, damping = 1e-6f, eps_rotation_rad = 1e-4f, eps_translation_m = 1e-4f;
    int max_iterations = 10, point_stride = 1, min_inliers = 64;
    uint32_t dof_mask = 0x3fu;
  };
  bool alignPointCloud(const vxb::Transformation& T_G_C, const vxb::Pointcloud& points_C, const AlignOptions& options,
                       vxb::Transformation* T_refined);
  const ks_align_stats& lastAlignStats() const { return last_align_stats_; }
  /// The object instances of the map (ks_objects_update; the contract is DESIGN.md, "Object instances"): the surface voxels of
  /// every label clustered into 26-connected components ON THE DEVICE, as the map is after the frames in flight.  Needs NO
  /// syncLayers(): the voxels stay in HBM, only the records travel.  What a scene-graph builder downstream of the reference does
  /// on the host from a synced layer.  surface_distance_m = 0: the voxel size.  Objects ascend by their smallest voxel (x, y, z).
  struct ObjectOptions {
    float min_weight = 1e-4f, surface_distance_m = 0.0f;
    uint32_t label_mask = 0x1fffffu, min_voxels = 8;
  };
  struct ObjectInstance {
    uint8_t label;
    uint32_t n_voxels;
    vxb::GlobalIndex first_voxel, bb_min, bb_max;   ///< global voxel indices, the box inclusive; first_voxel is the identity
    vxb::Point centroid;                            ///< metres, world frame
  };
  /// Returns true when `out` is not empty.
  bool extractObjects(const ObjectOptions& options, std::vector<ObjectInstance>* out);
  const ks_objects_stats& lastObjectsStats() const { return last_objects_stats_; }
  /// Where an explorer may go next (ks_frontiers_update; the contract is DESIGN.md, "Exploration frontiers"): the voxels of the
  /// STORED ESDF a sphere of radius_m may occupy that border space nobody has observed, clustered into 26-connected components ON THE
  /// DEVICE and joined with the navigation field, if updateNavField() has stored one.  Call updateEsdf() / refreshEsdf() first.
  /// Frontiers ascend by their smallest voxel (x, y, z).  The bounds are inclusive global voxel indices.
  struct FrontierOptions {
    float radius_m = 0.3f;
    uint32_t min_voxels = 8;
    bool use_bounds = false;
    vxb::GlobalIndex bounds_min = vxb::GlobalIndex(0, 0, 0), bounds_max = vxb::GlobalIndex(0, 0, 0);
  };
  struct Frontier {
    vxb::Point centroid;   ///< metres, world frame
    vxb::Point target;     ///< metres: the centre of record.nav_voxel, a valid start for planPaths()
    ks_frontier record;    ///< nav_cost is KS_NAV_UNREACHED when the field does not reach it, or none is stored
  };
  /// Returns true when `out` is not empty.
  bool extractFrontiers(const FrontierOptions& options, std::vector<Frontier>* out);
  const ks_frontier_stats& lastFrontierStats() const { return last_frontier_stats_; }
  /// The rooms of the map (ks_rooms_update; the contract is DESIGN.md, "Rooms"): the voxels of the STORED ESDF at least
  /// core_distance_m from every surface clustered into 26-connected components ON THE DEVICE (free space falls apart at doors),
  /// every other free voxel handed to the room nearest through free space, the contacts between rooms as links, and the objects of
  /// the last extractObjects() joined: room_of_object[i] is the room of object i, or KS_ROOM_NONE.  Call updateEsdf() / refreshEsdf()
  /// first.  Rooms ascend by their smallest core voxel (x, y, z), links by (room_a, room_b).  The bounds are inclusive global voxel indices.
  struct RoomOptions {
    float free_distance_m = 0.0f, core_distance_m = 0.5f;
    uint32_t min_core_voxels = 64;
    uint32_t max_cost = 0;          ///< 0: KS_NAV_MAX_COST
    bool use_bounds = false;
    vxb::GlobalIndex bounds_min = vxb::GlobalIndex(0, 0, 0), bounds_max = vxb::GlobalIndex(0, 0, 0);
  };
  struct Room {
    vxb::Point centroid;   ///< metres, world frame, over the assigned voxels: may lie inside a wall of an L-shaped room
    vxb::Point centre;     ///< metres: the centre of record.centre_voxel, always free: a valid goal for updateNavField()
    float clearance_m;     ///< the largest stored distance among its core voxels
    ks_room record;
  };
  struct RoomLink {
    vxb::Point door;       ///< metres: the centre of record.door_voxel
    float half_width_m;    ///< the largest stored distance among the contacts
    ks_room_link record;
  };
  /// Returns true when `rooms` is not empty.  links and room_of_object may be nullptr.
  bool segmentRooms(const RoomOptions& options, std::vector<Room>* rooms, std::vector<RoomLink>* links, std::vector<uint32_t>* room_of_object);
  const ks_rooms_stats& lastRoomsStats() const { return last_rooms_stats_; }
  /// How much unobserved space each candidate camera pose would see (ks_view_gain; the contract is DESIGN.md, "View information
  /// gain"): the distinct unknown, free and surface voxels of the STORED ESDF that the rays of a small pinhole image visit before a
  /// surface stops them, counted ON THE DEVICE.  Call updateEsdf() / refreshEsdf() first.  One record per pose, in the order of the poses;
  /// a pose with a non-finite component gets an all-zero record.
  struct ViewGainOptions {
    float min_range_m = 0.0f, max_range_m = 5.0f;
    float step_m = 0.0f;            ///< 0: the voxel size
    float stop_distance_m = 0.0f;
    uint32_t width = 32, height = 24;
    float fx = 0.0f, fy = 0.0f, cx = 0.0f, cy = 0.0f;   ///< no default: the caller sets them
    uint32_t label = 255;           ///< 255: no label is counted
  };
  /// Returns true when `out` is not empty.
  bool scoreViews(const std::vector<vxb::Transformation>& T_G_C, const ViewGainOptions& options, std::vector<ks_view_gain_record>* out);
  const ks_view_gain_stats& lastViewGainStats() const { return last_view_gain_stats_; }
  /// Fuses the map of another integrator into this one at a rigid pose ON THE DEVICE (ks_fuse_map; the contract is DESIGN.md,
  /// section 17): the submap's TSDF and semantics are resampled under T_G_S (submap frame -> this map's frame) into this map's grid and
  /// folded in by the layer-merge rule — what a server does with a layer it receives on Voxblox's tsdf_map_in
  /// (mergeLayerAintoLayerB(layer, T, ...)), or a submap mapper after a loop closure or alignPointCloud corrected the submap's pose.
  /// Both integrators complete their frames in flight; the submap is only read (neither its device map nor its host layers change).
  /// The touched tiles are flagged like integrated ones, so this integrator's host layers follow by its sync policy: at once under
  /// kEveryFrame, at the next syncLayers() under kOnDemand.  Both must have the same voxel size and live on the same device; their
  /// voxels_per_side may differ.  Returns true when at least one voxel was fused.
  struct FuseOptions {
    float min_weight = 1e-4f;
    uint64_t max_workspace_bytes = 1ull << 30;
  };
  bool fuseSubmap(HipSemanticTsdfIntegrator& submap, const vxb::Transformation& T_G_S, const FuseOptions& options);
  const ks_fuse_stats& lastFuseStats() const { return last_fuse_stats_; }
  SyncPolicy syncPolicy() const { return options_.sync_policy; }

  ks_ctx* context() { return ctx_; }
  const ks_frame_stats& lastFrameStats() const { return last_stats_; }

 private:
  void check(int rc, const char* what) const;
  ks_ctx* ctx_ = nullptr;
  Method method_;
  DeviceOptions options_;
  ks_frame_stats last_stats_{};
  ks_mesh_stats last_mesh_stats_{};
  ks_esdf_stats last_esdf_stats_{};
  ks_esdf_sample_stats last_esdf_sample_stats_{};
  ks_esdf_sweep_stats last_esdf_sweep_stats_{};
  ks_nav_stats last_nav_stats_{};
  ks_nav_path_stats last_nav_path_stats_{};
  ks_path_shorten_stats last_path_shorten_stats_{};
  ks_esdf_refresh_stats last_esdf_refresh_stats_{};
  ks_render_stats last_render_stats_{};
  ks_align_stats last_align_stats_{};
  ks_objects_stats last_objects_stats_{};
  ks_frontier_stats last_frontier_stats_{};
  ks_rooms_stats last_rooms_stats_{};
  ks_view_gain_stats last_view_gain_stats_{};
  ks_remove_stats last_remove_stats_{};
  ks_fuse_stats last_fuse_stats_{};
  vxb::FloatingPoint prune_distance_ = std::numeric_limits<vxb::FloatingPoint>::max();
  bool prune_keep_semantic_ = true;
  void pruneAfterFrame(const vxb::Transformation& T_G_C) {
    if (prune_distance_ < std::numeric_limits<vxb::FloatingPoint>::max()) removeDistantBlocks(T_G_C.getPosition(), prune_distance_, prune_keep_semantic_);
  }
  void downloadEsdfBlocks(const std::vector<int32_t>& idx, std::vector<EsdfBlock>* out);
  vxb::Layer<SemanticVoxel>* semantic_layer_ptr_;
  // page-locked staging for layer transfers (ks_host_alloc); grows on demand
  struct Staging {
    uint8_t* p = nullptr;
    size_t cap = 0;
    uint8_t* reserve(size_t bytes);
    ~Staging();
  };
  std::vector<int32_t> idx_buf_;
  Staging tsdf_buf_, sem_buf_, vox_buf_, run_buf_;

  /// Persistent workers for the scatter of downloaded voxels into the host layers (thread start-up per frame
  /// costs as much as the scatter itself).
  class Workers {
   public:
    ~Workers();
    /// fn(begin, end) over [0, n) cut into `parts` ranges; returns when all ranges are done.
    void run(size_t n, size_t parts, const std::function<void(size_t, size_t)>& fn);

   private:
    void loop(size_t id);
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_work_, cv_done_;
    const std::function<void(size_t, size_t)>* fn_ = nullptr;
    size_t n_ = 0, parts_ = 0, next_ = 0, pending_ = 0;
    uint64_t epoch_ = 0;
    bool stop_ = false;
  };
  Workers workers_;
};

/// Same shape as kimera::SemanticTsdfIntegratorFactory
/// (kimera_semantics/include/kimera_semantics/semantic_tsdf_integrator_factory.h:57-100):
/// "fast" / "merged" (and the explicit aliases "fast_hip" / "merged_hip") return the HIP
/// integrator as std::unique_ptr<vxb::TsdfIntegratorBase>; anything else is LOG(FATAL).
class HipSemanticTsdfIntegratorFactory {
 public:
  static std::unique_ptr<vxb::TsdfIntegratorBase> create(
      const std::string& integrator_type_name, const vxb::TsdfIntegratorBase::Config& config,
      const SemanticIntegratorBase::SemanticConfig& semantic_config, vxb::Layer<vxb::TsdfVoxel>* tsdf_layer,
      vxb::Layer<SemanticVoxel>* semantic_layer,
      const HipSemanticTsdfIntegrator::DeviceOptions& options = HipSemanticTsdfIntegrator::DeviceOptions());

  /// The enum overload of the reference factory (semantic_tsdf_integrator_factory.h:84-93): kMerged = 0, kFast = 1,
  /// plus the values integration/factory.patch adds for the explicit names, kMergedHip = 2, kFastHip = 3.  Taken
  /// as the enum's underlying int so that this header does not depend on the (patched) factory header;
  /// anything else is LOG(FATAL), like the reference's default branch (semantic_tsdf_integrator_factory.cpp:82-86).
  static std::unique_ptr<vxb::TsdfIntegratorBase> create(
      int integrator_type, const vxb::TsdfIntegratorBase::Config& config,
      const SemanticIntegratorBase::SemanticConfig& semantic_config, vxb::Layer<vxb::TsdfVoxel>* tsdf_layer,
      vxb::Layer<SemanticVoxel>* semantic_layer,
      const HipSemanticTsdfIntegrator::DeviceOptions& options = HipSemanticTsdfIntegrator::DeviceOptions());
  template <typename Enum, typename = typename std::enable_if<std::is_enum<Enum>::value>::type>
  static std::unique_ptr<vxb::TsdfIntegratorBase> create(
      const Enum& integrator_type, const vxb::TsdfIntegratorBase::Config& config,
      const SemanticIntegratorBase::SemanticConfig& semantic_config, vxb::Layer<vxb::TsdfVoxel>* tsdf_layer,
      vxb::Layer<SemanticVoxel>* semantic_layer,
      const HipSemanticTsdfIntegrator::DeviceOptions& options = HipSemanticTsdfIntegrator::DeviceOptions()) {
    return create(static_cast<int>(integrator_type), config, semantic_config, tsdf_layer, semantic_layer, options);
  }

 private:
  HipSemanticTsdfIntegratorFactory() = default;
};

}  // namespace kimera
