// adapter_demo — drives the C++ adapter exactly as SemanticTsdfServer would: build Layers,
// create the integrator through the factory, feed colour-encoded clouds through the
// TsdfIntegratorBase virtual, then dump the host Layers.  Used by tests/test_host_adapter_gpu.py.
//   adapter_demo <method> <labels.csv> <in.bin> <out.bin> [color_mode] [max_consecutive_ray_collisions] [restart_after] [pipeline]
// pipeline = 1: the patched server's sequence — factory with default options, THEN setSyncPolicy(kOnDemand) — frames
// overlap on the GPU, the host Layers are filled by one syncLayers() at the end, as a mesh timer would.
// restart_after = k: after frame k the integrator is destroyed and a new one is created on the
// same, now non-empty, Layers (the loadMap / re-configure case): it must pick the map up from the host.
// in.bin : u32 n_frames, then per frame { f32 T[7]; u32 n; f32 xyz[3n]; u8 rgba[4n] }
// out.bin: u32 n_blocks, u32 vps, then per block { i32 idx[3]; tsdf vps^3*12 B; semantic vps^3*92 B }
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <voxblox/utils/timing.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "hip_semantic_tsdf_integrator.h"
#ifdef KS_DEMO_REAL_FACTORY
#include <kimera_semantics/semantic_tsdf_integrator_factory.h>
#endif

namespace vxb = voxblox;

int main(int argc, char** argv) {
#ifdef KS_DEMO_REAL_FACTORY
  // (tests) which of its two permutations the reference-side Voxblox shim's "mixed" index produces — the adapter must
  // FIND OUT, it is not told (oracle/ref_shim/voxblox/integrator/integrator_utils.h)
  if (const char* form = std::getenv("KS_DEMO_SHIM_MIXED_FORM")) vxb::shim_mixed_order_form() = std::atoi(form);
#endif
  if (argc >= 2 && std::string(argv[1]) == "--probe-order") {
    // what HipSemanticTsdfIntegrator::probeMixedOrder() reads from the ThreadSafeIndexFactory of this build (no GPU needed)
    std::printf("probeMixedOrder: %d\n", kimera::HipSemanticTsdfIntegrator::probeMixedOrder());
    return 0;
  }
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s method labels.csv in.bin out.bin [color_mode] [max_collisions]\n", argv[0]);
    return 2;
  }
  const std::string method = argv[1];
  vxb::TsdfIntegratorBase::Config cfg;
  cfg.default_truncation_distance = 0.2f;  // voxblox_ros: 4 x voxel size
  cfg.max_ray_length_m = 5.0f;
  cfg.integrator_threads = 1;  // (only the reference's CPU integrators read it: one thread = their deterministic order)
  if (argc > 6) cfg.max_consecutive_ray_collisions = std::atoi(argv[6]);
  if (const char* b = std::getenv("KS_DEMO_MAX_INTEGRATION_TIME_S")) cfg.max_integration_time_s = (float)std::atof(b);  // (tests)
  kimera::SemanticIntegratorBase::SemanticConfig sc;
  sc.semantic_measurement_probability_ = 0.8f;
  sc.color_mode = static_cast<kimera::ColorMode>(argc > 5 ? std::atoi(argv[5]) : 1);
  sc.semantic_label_to_color_ = std::make_shared<kimera::SemanticLabel2Color>(argv[2]);
  sc.dynamic_labels_.push_back(20);
  vxb::Layer<vxb::TsdfVoxel> tsdf_layer(0.05f, 16);
  vxb::Layer<kimera::SemanticVoxel> semantic_layer(0.05f, 16);
  kimera::HipSemanticTsdfIntegrator::DeviceOptions opt;
  opt.max_tiles = 4096;
  opt.max_points = 1u << 18;
  if (const char* pf = std::getenv("KS_DEMO_PIPELINE_FRAMES")) opt.pipeline_frames = std::atoi(pf);  // (tests: DeviceOptions::pipeline_frames, 0 .. 16)
  // pipeline != 0: the sequence of a server with integration/server.patch — the factory hands the integrator out with its
  // default options (strict policy), THEN the server selects kOnDemand and syncs where it reads the Layers
  const bool pipeline = argc > 8 && std::atoi(argv[8]) != 0;
#ifdef KS_DEMO_REAL_FACTORY
  // integration/build_real_kimera.sh: the REAL kimera::SemanticTsdfIntegratorFactory (reference source +
  // integration/factory.patch) hands the integrator out, as SemanticTsdfServer's constructor gets it
  // (kimera_semantics_ros/src/semantic_tsdf_server.cpp:71-78); "enum:<n>" goes through the enum overload.
  auto make = [&]() -> std::unique_ptr<vxb::TsdfIntegratorBase> {
    if (method.rfind("enum:", 0) == 0)
      return kimera::SemanticTsdfIntegratorFactory::create(static_cast<kimera::SemanticTsdfIntegratorType>(std::atoi(method.c_str() + 5)),
                                                          cfg, sc, &tsdf_layer, &semantic_layer);
    return kimera::SemanticTsdfIntegratorFactory::create(method, cfg, sc, &tsdf_layer, &semantic_layer);
  };
#else
  auto make = [&]() -> std::unique_ptr<vxb::TsdfIntegratorBase> {
    if (method.rfind("enum:", 0) == 0)
      return kimera::HipSemanticTsdfIntegratorFactory::create(std::atoi(method.c_str() + 5), cfg, sc, &tsdf_layer, &semantic_layer, opt);
    return kimera::HipSemanticTsdfIntegratorFactory::create(method, cfg, sc, &tsdf_layer, &semantic_layer, opt);
  };
#endif
  std::unique_ptr<vxb::TsdfIntegratorBase> integrator = make();
  // KS_DEMO_FUSE="qw qx qy qz tx ty tz": a submap mapper — the first half of the frames goes into a SUBMAP integrator with layers of
  // its own, the rest into the main one; then the submap is fused into the main map at the given pose (fuseSubmap: resampled and
  // merged on the device) and the main integrator's host layers, which follow by its sync policy, are dumped
  vxb::Layer<vxb::TsdfVoxel> sub_tsdf_layer(0.05f, 16);
  vxb::Layer<kimera::SemanticVoxel> sub_semantic_layer(0.05f, 16);
  std::unique_ptr<vxb::TsdfIntegratorBase> submap;
  float fuse_T[7] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (const char* fp = std::getenv("KS_DEMO_FUSE")) {
    if (std::sscanf(fp, "%f %f %f %f %f %f %f", &fuse_T[0], &fuse_T[1], &fuse_T[2], &fuse_T[3], &fuse_T[4], &fuse_T[5], &fuse_T[6]) != 7) return 2;
#ifdef KS_DEMO_REAL_FACTORY
    submap = kimera::SemanticTsdfIntegratorFactory::create(method, cfg, sc, &sub_tsdf_layer, &sub_semantic_layer);
#else
    submap = kimera::HipSemanticTsdfIntegratorFactory::create(method, cfg, sc, &sub_tsdf_layer, &sub_semantic_layer, opt);
#endif
    if (pipeline)
      if (auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(submap.get())) hip->setSyncPolicy(kimera::HipSemanticTsdfIntegrator::SyncPolicy::kOnDemand);
  }
  auto on_demand = [&]() {
    if (!pipeline) return;
    if (auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get()))
      hip->setSyncPolicy(kimera::HipSemanticTsdfIntegrator::SyncPolicy::kOnDemand);
  };
  on_demand();
  // KS_DEMO_PRUNE=<metres>: vxb::TsdfServer with max_block_distance_from_body, as integration/server.patch wires it — the server
  // hands its radius to the integrator once, and every integrated cloud ends with removeDistantBlocks around the sensor: the
  // far blocks leave the device map and the host TSDF layer.  KS_DEMO_PRUNE_DROP_SEMANTIC=1: and the host semantic layer
  auto pruning = [&]() {
    const char* prune = std::getenv("KS_DEMO_PRUNE");
    if (!prune) return;
    const char* drop = std::getenv("KS_DEMO_PRUNE_DROP_SEMANTIC");
    if (auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get()))
      hip->setMaxBlockDistanceFromBody((float)std::atof(prune), /*keep_semantic_layer=*/!(drop && std::atoi(drop) != 0));
  };
  pruning();
  if (auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get())) {
    int32_t shape[4] = {0, 0, 0, 0};
    ks_pipeline_shape(hip->context(), shape);
    std::printf("adapter_demo: pipeline shape: lag %d slots %d batch %d march streams %d\n", shape[0], shape[1], shape[2], shape[3]);
  }

  FILE* in = std::fopen(argv[3], "rb");
  if (!in) return 3;
  uint32_t n_frames = 0;
  if (std::fread(&n_frames, 4, 1, in) != 1) return 3;
  const int restart_after = argc > 7 ? std::atoi(argv[7]) : -1;
  double integrate_ms = 0.0, tail_ms = 0.0;
  uint32_t tail_frames = 0;
  // KS_DEMO_ESDF_REFRESH=<file>: an ESDF kept up to date while frames stream in — updateEsdf after the first half of the
  // frames, refreshEsdf after the last, which hands back only the blocks it recomputed
  const char* esdf_refresh_path = std::getenv("KS_DEMO_ESDF_REFRESH");
  using EsdfBlock = kimera::HipSemanticTsdfIntegrator::EsdfBlock;
  std::map<std::array<int32_t, 3>, EsdfBlock> esdf_kept;   // (ascending by x, y, z)
  float last_T[7] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // pose of the last frame read (KS_DEMO_RENDER, KS_DEMO_ALIGN)
  vxb::Pointcloud last_points;                                     // ... and its cloud (KS_DEMO_ALIGN)
  for (uint32_t f = 0; f < n_frames; ++f) {
    if (esdf_refresh_path && f == n_frames / 2) {
      auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
      if (!hip) return 8;
      kimera::HipSemanticTsdfIntegrator::EsdfOptions eo;
      eo.min_distance_m = 0.1f;
      eo.max_distance_m = 0.4f;
      std::vector<EsdfBlock> esdf;
      hip->updateEsdf(eo, &esdf);
      for (auto& eb : esdf) esdf_kept[{eb.index.x(), eb.index.y(), eb.index.z()}] = std::move(eb);
      std::printf("adapter_demo: updateEsdf after %u frames, %zu blocks\n", f, esdf_kept.size());
    }
    if ((int)f == restart_after) {
      if (pipeline)   // (a server syncs before it lets go of the integrator: the Layers are what the next one starts from)
        if (auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get())) hip->syncLayers();
      integrator.reset();
      integrator = make();
      on_demand();
      pruning();
    }
    if (const char* ca = std::getenv("KS_DEMO_CLEAR_AFTER")) {
      if ((int)f == std::atoi(ca)) {
        // SemanticTsdfServer::clear() with integration/server.patch: sync, the base class removes the TSDF blocks (the
        // semantic layer and the integrator survive), the GPU map follows
        auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
        if (!hip) return 7;
        hip->syncLayers();
        tsdf_layer.removeAllBlocks();   // vxb::TsdfServer::clear()
        hip->clearDeviceMap(/*keep_integrator_state=*/true);
        hip->uploadLayers();
      }
    }
    float T[7];
    uint32_t n;
    if (std::fread(T, 4, 7, in) != 7 || std::fread(&n, 4, 1, in) != 1) return 3;
    std::memcpy(last_T, T, sizeof(T));
    vxb::Pointcloud pts(n);
    vxb::Colors cols(n);
    std::vector<float> xyz(3 * size_t(n));
    std::vector<uint8_t> rgba(4 * size_t(n));
    if (std::fread(xyz.data(), 4, xyz.size(), in) != xyz.size() || std::fread(rgba.data(), 1, rgba.size(), in) != rgba.size()) return 3;
    for (uint32_t i = 0; i < n; ++i) {
      pts[i] = vxb::Point(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
      cols[i] = vxb::Color(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]);
    }
    if (f + 1 == n_frames && std::getenv("KS_DEMO_ALIGN")) last_points = pts;
    const auto t0 = std::chrono::steady_clock::now();
    (submap && 2 * f < n_frames ? submap : integrator)->integratePointCloud(vxb::Transformation(T[0], T[1], T[2], T[3], vxb::Point(T[4], T[5], T[6])), pts, cols, false);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    integrate_ms += ms;
    if (std::getenv("KS_DEMO_PRUNE")) {
      auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
      if (!hip) return 7;
      const ks_remove_stats& rs = hip->lastRemoveStats();
      std::printf("adapter_demo: pruned after frame %u: %llu blocks removed, %llu tiles resident of a pool of %llu, host layers %zu tsdf / %zu semantic blocks\n",
                  f, (unsigned long long)rs.blocks_removed, (unsigned long long)rs.tiles_resident, (unsigned long long)rs.pool_capacity_tiles,
                  tsdf_layer.getNumberOfAllocatedBlocks(), semantic_layer.getNumberOfAllocatedBlocks());
    }
    if (std::getenv("KS_DEMO_TRACE")) std::fprintf(stderr, "frame %u done (%.3f ms, %zu blocks)\n", f, ms, tsdf_layer.getNumberOfAllocatedBlocks());
    if (3 * f >= 2 * n_frames) {  // steady state: the last third (staging buffers and most blocks exist)
      tail_ms += ms;
      ++tail_frames;
    }
  }
  std::fclose(in);
  if (submap) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    auto* sub = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(submap.get());
    if (!hip || !sub) return 7;
    const auto t0 = std::chrono::steady_clock::now();
    hip->fuseSubmap(*sub, vxb::Transformation(fuse_T[0], fuse_T[1], fuse_T[2], fuse_T[3], vxb::Point(fuse_T[4], fuse_T[5], fuse_T[6])),
                    kimera::HipSemanticTsdfIntegrator::FuseOptions());
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const ks_fuse_stats& fs = hip->lastFuseStats();
    std::printf("adapter_demo: fuseSubmap %.3f ms, %llu source tiles, %llu of %llu candidate tiles touched, %llu allocated, %llu voxels fused, submap host layers %zu blocks\n", ms,
                (unsigned long long)fs.tiles_source, (unsigned long long)fs.tiles_touched, (unsigned long long)fs.tiles_candidate,
                (unsigned long long)fs.tiles_allocated, (unsigned long long)fs.voxels_fused, sub_tsdf_layer.getNumberOfAllocatedBlocks());
  }
  if (pipeline) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip) return 7;
    const auto t0 = std::chrono::steady_clock::now();
    hip->syncLayers();
    std::printf("adapter_demo: final syncLayers %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  if (n_frames)
    std::printf("adapter_demo: integratePointCloud %.3f ms/frame over %u frames, %.3f ms/frame over the last %u (host clouds, %s)\n",
                integrate_ms / n_frames, n_frames, tail_frames ? tail_ms / tail_frames : 0.0, tail_frames,
                pipeline ? "kOnDemand + pipeline_frames" : "kEveryFrame layer sync");

  // KS_DEMO_MESH=<file>: the semantic mesh, made on the device without any layer sync (updateMesh), written as
  // { u32 blocks; per block: i32 index[3], u32 n, n x Point vertices, n x Point normals, n x Color, n x u8 label }
  if (const char* mesh_path = std::getenv("KS_DEMO_MESH")) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip) return 8;
    std::vector<kimera::HipSemanticTsdfIntegrator::MeshBlock> changed;
    const auto t0 = std::chrono::steady_clock::now();
    hip->updateMesh(false, &changed);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE* mf = std::fopen(mesh_path, "wb");
    if (!mf) return 9;
    const uint32_t n_mesh_blocks = changed.size();
    std::fwrite(&n_mesh_blocks, 4, 1, mf);
    size_t n_vertices = 0;
    for (const auto& mb : changed) {
      const int32_t idx[3] = {mb.index.x(), mb.index.y(), mb.index.z()};
      const uint32_t n = mb.vertices.size();
      std::fwrite(idx, 4, 3, mf);
      std::fwrite(&n, 4, 1, mf);
      std::fwrite(mb.vertices.data(), sizeof(vxb::Point), n, mf);
      std::fwrite(mb.normals.data(), sizeof(vxb::Point), n, mf);
      std::fwrite(mb.colors.data(), sizeof(vxb::Color), n, mf);
      std::fwrite(mb.labels.data(), 1, n, mf);
      n_vertices += n;
    }
    std::fclose(mf);
    std::printf("adapter_demo: updateMesh %.3f ms, %u blocks, %zu triangles\n", ms, n_mesh_blocks, n_vertices / 3);
  }

  // KS_DEMO_MESH_INDEXED=<file>: that mesh with shared vertices (indexMesh, no layer sync either), written as
  // { u32 vertices, u32 indices; V x Point vertices, V x Point normals, V x Color, V x u8 label, V x u32 object id, C x u32 index }
  if (const char* indexed_path = std::getenv("KS_DEMO_MESH_INDEXED")) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip) return 8;
    std::vector<kimera::HipSemanticTsdfIntegrator::MeshBlock> changed;
    hip->updateMesh(true, &changed);   // (brings the stored mesh up to date: everything, if KS_DEMO_MESH has not made it)
    kimera::HipSemanticTsdfIntegrator::IndexedMesh im;
    const auto t0 = std::chrono::steady_clock::now();
    hip->indexMesh(&im);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE* mf = std::fopen(indexed_path, "wb");
    if (!mf) return 9;
    const uint32_t counts[2] = {(uint32_t)im.vertices.size(), (uint32_t)im.indices.size()};
    std::fwrite(counts, 4, 2, mf);
    std::fwrite(im.vertices.data(), sizeof(vxb::Point), counts[0], mf);
    std::fwrite(im.normals.data(), sizeof(vxb::Point), counts[0], mf);
    std::fwrite(im.colors.data(), sizeof(vxb::Color), counts[0], mf);
    std::fwrite(im.labels.data(), 1, counts[0], mf);
    std::fwrite(im.object_ids.data(), 4, counts[0], mf);
    std::fwrite(im.indices.data(), 4, counts[1], mf);
    std::fclose(mf);
    std::printf("adapter_demo: indexMesh %.3f ms, %u vertices for %u corners in %zu blocks, at most %llu corners on a vertex\n", ms, counts[0],
                counts[1], im.blocks.size(), (unsigned long long)im.stats.max_corners_per_vertex);
  }

  // KS_DEMO_ESDF=<file>: the batch ESDF with nearest-surface labels, made on the device without any layer sync (updateEsdf,
  // min_distance_m 0.1, max_distance_m 0.4), written as
  // { u32 blocks, u32 voxels_per_side; per block: i32 index[3], vps^3 x { f32 distance, u8 flags, u8 nearest_label, u8 pad[2] } }
  if (const char* esdf_path = std::getenv("KS_DEMO_ESDF")) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip) return 8;
    kimera::HipSemanticTsdfIntegrator::EsdfOptions eo;
    eo.min_distance_m = 0.1f;
    eo.max_distance_m = 0.4f;
    std::vector<kimera::HipSemanticTsdfIntegrator::EsdfBlock> esdf;
    const auto t0 = std::chrono::steady_clock::now();
    hip->updateEsdf(eo, &esdf);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE* ef = std::fopen(esdf_path, "wb");
    if (!ef) return 9;
    const uint32_t n_esdf_blocks = esdf.size(), esdf_vps = tsdf_layer.voxels_per_side();
    std::fwrite(&n_esdf_blocks, 4, 1, ef);
    std::fwrite(&esdf_vps, 4, 1, ef);
    for (const auto& eb : esdf) {
      const int32_t idx[3] = {eb.index.x(), eb.index.y(), eb.index.z()};
      std::fwrite(idx, 4, 3, ef);
      std::fwrite(eb.voxels.data(), sizeof(eb.voxels[0]), eb.voxels.size(), ef);
    }
    std::fclose(ef);
    const ks_esdf_stats& es = hip->lastEsdfStats();
    std::printf("adapter_demo: updateEsdf %.3f ms, %u blocks, %llu observed voxels, %llu in the band\n", ms, n_esdf_blocks,
                (unsigned long long)es.voxels_observed, (unsigned long long)es.voxels_fixed);
  }

  // KS_DEMO_ESDF_SAMPLE=<file>: what a planner reads of the ESDF, on the device without any layer sync — updateEsdf (min_distance_m
  // 0.1, max_distance_m 0.4), then sampleEsdf on a 13^3 lattice around the last frame's position and sweepEsdf (default options) from
  // that position to every seventh lattice point, written as { u32 points, u32 segments; points x f32[3]; f32 distance[points];
  // f32 gradient[points][3]; u8 status[points], label[points], flags[points]; segments x f32[6]; u8 status[segments];
  // f32 t_stop[segments], min_clearance[segments], t_min[segments] }
  if (const char* sample_path = std::getenv("KS_DEMO_ESDF_SAMPLE")) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip) return 8;
    kimera::HipSemanticTsdfIntegrator::EsdfOptions eo;
    eo.min_distance_m = 0.1f;
    eo.max_distance_m = 0.4f;
    std::vector<kimera::HipSemanticTsdfIntegrator::EsdfBlock> esdf;
    hip->updateEsdf(eo, &esdf);
    const vxb::Point o(last_T[4], last_T[5], last_T[6]);
    vxb::Pointcloud pts;
    std::vector<kimera::HipSemanticTsdfIntegrator::EsdfSegment> segs;
    for (int k = -6; k <= 6; ++k)
      for (int j = -6; j <= 6; ++j)
        for (int i = -6; i <= 6; ++i) {
          pts.push_back(vxb::Point(o.x() + 0.31f * (float)i, o.y() + 0.27f * (float)j, o.z() + 0.13f * (float)k));
          if (pts.size() % 7 == 0) segs.push_back({o, pts.back()});
        }
    kimera::HipSemanticTsdfIntegrator::EsdfSamples sm;
    kimera::HipSemanticTsdfIntegrator::EsdfSweeps sw;
    const auto t0 = std::chrono::steady_clock::now();
    hip->sampleEsdf(pts, &sm);
    hip->sweepEsdf(segs, kimera::HipSemanticTsdfIntegrator::SweepOptions(), &sw);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE* sf = std::fopen(sample_path, "wb");
    if (!sf) return 9;
    const uint32_t np = pts.size(), ns = segs.size();
    std::fwrite(&np, 4, 1, sf);
    std::fwrite(&ns, 4, 1, sf);
    std::fwrite(pts.data(), 12, np, sf);
    std::fwrite(sm.distance.data(), 4, np, sf);
    std::fwrite(sm.gradient.data(), 12, np, sf);
    std::fwrite(sm.status.data(), 1, np, sf);
    std::fwrite(sm.label.data(), 1, np, sf);
    std::fwrite(sm.flags.data(), 1, np, sf);
    std::fwrite(segs.data(), 24, ns, sf);
    std::fwrite(sw.status.data(), 1, ns, sf);
    std::fwrite(sw.t_stop.data(), 4, ns, sf);
    std::fwrite(sw.min_clearance.data(), 4, ns, sf);
    std::fwrite(sw.t_min.data(), 4, ns, sf);
    std::fclose(sf);
    const ks_esdf_sample_stats& ss = hip->lastEsdfSampleStats();
    const ks_esdf_sweep_stats& ws = hip->lastEsdfSweepStats();
    std::printf("adapter_demo: sampleEsdf + sweepEsdf %.3f ms, %u points (%llu interpolated, %llu nearest), %u segments (%llu free, %llu collision, %llu samples)\n",
                ms, np, (unsigned long long)ss.points_interpolated, (unsigned long long)ss.points_nearest, ns, (unsigned long long)ws.segments_free,
                (unsigned long long)ws.segments_collision, (unsigned long long)ws.samples);
  }

  // KS_DEMO_NAV=<file>: where the robot can go and how, on the device without any layer sync — updateEsdf (min_distance_m 0.1,
  // max_distance_m 0.4), updateNavField (radius 0.2 m) with the last frame's position and a point 0.6 m beside it as goals, then
  // planPaths (at most 96 waypoints) from a 13^3 lattice around that position, written as { u32 goals, u32 starts, u32 max_waypoints;
  // goals x f32[3]; starts x f32[3]; u8 status[starts]; u32 cost[starts]; u32 n_waypoints[starts]; the waypoints of every start
  // in turn, n_waypoints x f32[3] each }
  if (const char* nav_path = std::getenv("KS_DEMO_NAV")) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip) return 8;
    kimera::HipSemanticTsdfIntegrator::EsdfOptions eo;
    eo.min_distance_m = 0.1f;
    eo.max_distance_m = 0.4f;
    std::vector<kimera::HipSemanticTsdfIntegrator::EsdfBlock> esdf;
    hip->updateEsdf(eo, &esdf);
    const vxb::Point o(last_T[4], last_T[5], last_T[6]);
    vxb::Pointcloud goals, starts;
    goals.push_back(o);
    goals.push_back(vxb::Point(o.x() + 0.6f, o.y(), o.z()));
    for (int k = -6; k <= 6; ++k)
      for (int j = -6; j <= 6; ++j)
        for (int i = -6; i <= 6; ++i) starts.push_back(vxb::Point(o.x() + 0.31f * (float)i, o.y() + 0.27f * (float)j, o.z() + 0.13f * (float)k));
    kimera::HipSemanticTsdfIntegrator::NavOptions no;
    no.radius_m = 0.2f;
    kimera::HipSemanticTsdfIntegrator::NavPaths paths;
    const uint32_t max_waypoints = 96;
    const auto t0 = std::chrono::steady_clock::now();
    hip->updateNavField(goals, no);
    hip->planPaths(starts, max_waypoints, &paths);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE* nf = std::fopen(nav_path, "wb");
    if (!nf) return 9;
    const uint32_t ng = goals.size(), ns = starts.size();
    std::fwrite(&ng, 4, 1, nf);
    std::fwrite(&ns, 4, 1, nf);
    std::fwrite(&max_waypoints, 4, 1, nf);
    std::fwrite(goals.data(), 12, ng, nf);
    std::fwrite(starts.data(), 12, ns, nf);
    std::fwrite(paths.status.data(), 1, ns, nf);
    std::fwrite(paths.cost.data(), 4, ns, nf);
    for (const auto& w : paths.waypoints) {
      const uint32_t nw = w.size();
      std::fwrite(&nw, 4, 1, nf);
    }
    for (const auto& w : paths.waypoints) std::fwrite(w.data(), 12, w.size(), nf);
    std::fclose(nf);
    const ks_nav_stats& st = hip->lastNavStats();
    const ks_nav_path_stats& ps = hip->lastNavPathStats();
    std::printf("adapter_demo: updateNavField + planPaths %.3f ms, %llu of %llu traversable voxels reached in %llu rounds, %u starts (%llu reached, %llu unreachable, %llu blocked, %llu waypoints)\n",
                ms, (unsigned long long)st.voxels_reached, (unsigned long long)st.voxels_traversable, (unsigned long long)st.rounds, ns,
                (unsigned long long)ps.paths_reached, (unsigned long long)ps.paths_unreachable, (unsigned long long)ps.paths_blocked,
                (unsigned long long)ps.waypoints);
    // ... and KS_DEMO_SHORTEN=<file>: those paths pulled taut by line of sight (shortenPaths, the same radius, lookahead 48), written
    // as { u32 paths, u32 lookahead; u8 status[paths]; u32 n_waypoints[paths]; f32 length[paths]; f32 min_clearance[paths]; the
    // waypoints of every path in turn, n_waypoints x f32[3] each }; the paths that went in are those of the KS_DEMO_NAV file
    if (const char* shorten_path = std::getenv("KS_DEMO_SHORTEN")) {
      kimera::HipSemanticTsdfIntegrator::ShortenOptions so;
      so.radius_m = no.radius_m;
      so.lookahead = 48;
      kimera::HipSemanticTsdfIntegrator::ShortPaths taut;
      const auto t1 = std::chrono::steady_clock::now();
      hip->shortenPaths(paths.waypoints, so, &taut);
      const double ms1 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
      FILE* sf = std::fopen(shorten_path, "wb");
      if (!sf) return 9;
      std::fwrite(&ns, 4, 1, sf);
      std::fwrite(&so.lookahead, 4, 1, sf);
      std::fwrite(taut.status.data(), 1, ns, sf);
      for (const auto& w : taut.waypoints) {
        const uint32_t nw = w.size();
        std::fwrite(&nw, 4, 1, sf);
      }
      std::fwrite(taut.length.data(), 4, ns, sf);
      std::fwrite(taut.min_clearance.data(), 4, ns, sf);
      for (const auto& w : taut.waypoints) std::fwrite(w.data(), 12, w.size(), sf);
      std::fclose(sf);
      const ks_path_shorten_stats& hs = hip->lastPathShortenStats();
      std::printf("adapter_demo: shortenPaths %.3f ms, %llu -> %llu waypoints in %llu paths (%llu unverified, %llu invalid), %llu sweeps, %llu samples\n", ms1,
                  (unsigned long long)hs.waypoints_in, (unsigned long long)hs.waypoints_out, (unsigned long long)(hs.paths_ok + hs.paths_unverified),
                  (unsigned long long)hs.paths_unverified, (unsigned long long)hs.paths_invalid, (unsigned long long)hs.sweeps, (unsigned long long)hs.samples);
    }
  }

  // KS_DEMO_FRONTIERS=<file>: where an explorer may go next, on the device without any layer sync — updateEsdf (min_distance_m 0.1,
  // max_distance_m 0.4), updateNavField (radius 0.2 m) with the last frame's position as the one goal, then extractFrontiers (radius
  // 0.2 m, the other options default), written as { u32 frontiers; f32 goal[3]; u64 stats[9] (ks_frontier_stats); the 88-byte
  // records; per frontier f32 centroid[3], f32 target[3] }
  if (const char* frontiers_path = std::getenv("KS_DEMO_FRONTIERS")) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip) return 8;
    kimera::HipSemanticTsdfIntegrator::EsdfOptions eo;
    eo.min_distance_m = 0.1f;
    eo.max_distance_m = 0.4f;
    std::vector<kimera::HipSemanticTsdfIntegrator::EsdfBlock> esdf;
    hip->updateEsdf(eo, &esdf);
    vxb::Pointcloud goals;
    goals.push_back(vxb::Point(last_T[4], last_T[5], last_T[6]));
    kimera::HipSemanticTsdfIntegrator::NavOptions no;
    no.radius_m = 0.2f;
    hip->updateNavField(goals, no);
    kimera::HipSemanticTsdfIntegrator::FrontierOptions fo;
    fo.radius_m = 0.2f;
    std::vector<kimera::HipSemanticTsdfIntegrator::Frontier> frontiers;
    const auto t0 = std::chrono::steady_clock::now();
    hip->extractFrontiers(fo, &frontiers);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE* ff = std::fopen(frontiers_path, "wb");
    if (!ff) return 9;
    const uint32_t n_frontiers = frontiers.size();
    const ks_frontier_stats& fs = hip->lastFrontierStats();
    std::fwrite(&n_frontiers, 4, 1, ff);
    std::fwrite(goals.data(), 12, 1, ff);
    std::fwrite(&fs, sizeof(fs), 1, ff);
    for (const auto& f : frontiers) std::fwrite(&f.record, sizeof(ks_frontier), 1, ff);
    uint32_t reached = 0;
    for (const auto& f : frontiers) {
      const float m[6] = {f.centroid.x(), f.centroid.y(), f.centroid.z(), f.target.x(), f.target.y(), f.target.z()};
      std::fwrite(m, 4, 6, ff);
      reached += f.record.nav_cost <= KS_NAV_MAX_COST;
    }
    std::fclose(ff);
    std::printf("adapter_demo: extractFrontiers %.3f ms, %u frontiers of %llu components, %llu of %llu frontier voxels in them, %u reached by the field\n", ms,
                n_frontiers, (unsigned long long)fs.components, (unsigned long long)fs.voxels_in_frontiers, (unsigned long long)fs.voxels_frontier, reached);
  }

  // KS_DEMO_ROOMS=<file>: the rooms of the map, on the device without any layer sync — updateEsdf (min_distance_m 0.1, max_distance_m
  // 0.4), extractObjects (default options), then segmentRooms (core_distance_m 0.3, min_core_voxels 8, the other options default),
  // written as { u32 rooms, links, objects, 0; u64 stats[15] (ks_rooms_stats); the 96-byte records; the 32-byte links; u32
  // room_of_object[objects]; per room f32 centroid[3], centre[3], clearance_m; per link f32 door[3], half_width_m }
  if (const char* rooms_path = std::getenv("KS_DEMO_ROOMS")) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip) return 8;
    kimera::HipSemanticTsdfIntegrator::EsdfOptions eo;
    eo.min_distance_m = 0.1f;
    eo.max_distance_m = 0.4f;
    std::vector<kimera::HipSemanticTsdfIntegrator::EsdfBlock> esdf;
    hip->updateEsdf(eo, &esdf);
    std::vector<kimera::HipSemanticTsdfIntegrator::ObjectInstance> objects;
    hip->extractObjects(kimera::HipSemanticTsdfIntegrator::ObjectOptions(), &objects);
    kimera::HipSemanticTsdfIntegrator::RoomOptions ro;
    ro.core_distance_m = 0.3f;
    ro.min_core_voxels = 8;
    std::vector<kimera::HipSemanticTsdfIntegrator::Room> rooms;
    std::vector<kimera::HipSemanticTsdfIntegrator::RoomLink> links;
    std::vector<uint32_t> room_of_object;
    const auto t0 = std::chrono::steady_clock::now();
    hip->segmentRooms(ro, &rooms, &links, &room_of_object);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE* rf = std::fopen(rooms_path, "wb");
    if (!rf) return 9;
    const uint32_t head[4] = {(uint32_t)rooms.size(), (uint32_t)links.size(), (uint32_t)room_of_object.size(), 0u};
    const ks_rooms_stats& rs = hip->lastRoomsStats();
    std::fwrite(head, 4, 4, rf);
    std::fwrite(&rs, sizeof(rs), 1, rf);
    for (const auto& r : rooms) std::fwrite(&r.record, sizeof(ks_room), 1, rf);
    for (const auto& l : links) std::fwrite(&l.record, sizeof(ks_room_link), 1, rf);
    if (!room_of_object.empty()) std::fwrite(room_of_object.data(), 4, room_of_object.size(), rf);
    for (const auto& r : rooms) {
      const float m[7] = {r.centroid.x(), r.centroid.y(), r.centroid.z(), r.centre.x(), r.centre.y(), r.centre.z(), r.clearance_m};
      std::fwrite(m, 4, 7, rf);
    }
    for (const auto& l : links) {
      const float m[4] = {l.door.x(), l.door.y(), l.door.z(), l.half_width_m};
      std::fwrite(m, 4, 4, rf);
    }
    std::fclose(rf);
    std::printf("adapter_demo: segmentRooms %.3f ms, %u rooms of %llu core components, %u links, %llu of %llu free voxels assigned, %llu of %llu objects joined\n",
                ms, head[0], (unsigned long long)rs.components, head[1], (unsigned long long)rs.voxels_assigned, (unsigned long long)rs.voxels_free,
                (unsigned long long)rs.objects_joined, (unsigned long long)rs.objects_seen);
  }

  // KS_DEMO_VIEW_GAIN=<file>: how much unobserved space candidate views would see, on the device without any layer sync — updateEsdf
  // (min_distance_m 0.1, max_distance_m 0.4), then scoreViews for the last frame's pose turned about the world's z axis in 8 steps of
  // 45 degrees: 16 x 12 rays of a 90-degree image, 3 m range, label 4 counted; written as { u32 views, width, height, label; f32 K[4];
  // f32 max_range_m; u32 0; u64 stats[11] (ks_view_gain_stats); the poses (7 f32 each); the 32-byte records }
  if (const char* gain_path = std::getenv("KS_DEMO_VIEW_GAIN")) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip) return 8;
    kimera::HipSemanticTsdfIntegrator::EsdfOptions eo;
    eo.min_distance_m = 0.1f;
    eo.max_distance_m = 0.4f;
    std::vector<kimera::HipSemanticTsdfIntegrator::EsdfBlock> esdf;
    hip->updateEsdf(eo, &esdf);
    kimera::HipSemanticTsdfIntegrator::ViewGainOptions vo;
    vo.max_range_m = 3.0f;
    vo.width = 16;
    vo.height = 12;
    vo.fx = vo.fy = 8.0f;
    vo.cx = 7.5f;
    vo.cy = 5.5f;
    vo.label = 4;
    std::vector<vxb::Transformation> views;
    std::vector<float> poses;
    for (int k = 0; k < 8; ++k) {
      const double half = 0.5 * k * 0.78539816339744831, cz = std::cos(half), sz = std::sin(half);
      const double q[4] = {last_T[0], last_T[1], last_T[2], last_T[3]};
      // (cz, 0, 0, sz) * q: the camera's orientation turned about the world's z axis
      const float p[7] = {static_cast<float>(cz * q[0] - sz * q[3]), static_cast<float>(cz * q[1] - sz * q[2]), static_cast<float>(cz * q[2] + sz * q[1]),
                          static_cast<float>(cz * q[3] + sz * q[0]), last_T[4], last_T[5], last_T[6]};
      views.push_back(vxb::Transformation(p[0], p[1], p[2], p[3], vxb::Point(p[4], p[5], p[6])));
      const vxb::Transformation& T = views.back();   // (what scoreViews reads)
      const float back[7] = {T.qw(), T.qvec().x(), T.qvec().y(), T.qvec().z(), T.getPosition().x(), T.getPosition().y(), T.getPosition().z()};
      poses.insert(poses.end(), back, back + 7);
    }
    std::vector<ks_view_gain_record> records;
    const auto t0 = std::chrono::steady_clock::now();
    hip->scoreViews(views, vo, &records);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE* gf = std::fopen(gain_path, "wb");
    if (!gf) return 9;
    const uint32_t head[4] = {static_cast<uint32_t>(views.size()), vo.width, vo.height, vo.label};
    const float K[4] = {vo.fx, vo.fy, vo.cx, vo.cy};
    const uint32_t zero = 0;
    const ks_view_gain_stats& gs = hip->lastViewGainStats();
    std::fwrite(head, 4, 4, gf);
    std::fwrite(K, 4, 4, gf);
    std::fwrite(&vo.max_range_m, 4, 1, gf);
    std::fwrite(&zero, 4, 1, gf);
    std::fwrite(&gs, sizeof(gs), 1, gf);
    std::fwrite(poses.data(), 4, poses.size(), gf);
    std::fwrite(records.data(), sizeof(ks_view_gain_record), records.size(), gf);
    std::fclose(gf);
    size_t best = 0;
    for (size_t i = 1; i < records.size(); ++i)
      if (records[i].unknown_voxels > records[best].unknown_voxels) best = i;
    std::printf("adapter_demo: scoreViews %.3f ms, %zu views, %llu unknown / %llu free / %llu surface voxels in all, the best view (%zu) sees %u unknown voxels\n", ms,
                records.size(), (unsigned long long)gs.unknown_voxels, (unsigned long long)gs.free_voxels, (unsigned long long)gs.surface_voxels, best,
                records.empty() ? 0u : records[best].unknown_voxels);
  }

  // KS_DEMO_OBJECTS=<file>: the object instances of the map, made on the device without any layer sync (extractObjects,
  // default options), written as { u32 objects; per object: u32 label, u32 n_voxels, i64 first_voxel[3], i64 bb_min[3],
  // i64 bb_max[3], f32 centroid[3] }
  if (const char* objects_path = std::getenv("KS_DEMO_OBJECTS")) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip) return 8;
    std::vector<kimera::HipSemanticTsdfIntegrator::ObjectInstance> objects;
    const auto t0 = std::chrono::steady_clock::now();
    hip->extractObjects(kimera::HipSemanticTsdfIntegrator::ObjectOptions(), &objects);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE* of = std::fopen(objects_path, "wb");
    if (!of) return 9;
    const uint32_t n_objects = objects.size();
    std::fwrite(&n_objects, 4, 1, of);
    for (const auto& o : objects) {
      const uint32_t head[2] = {o.label, o.n_voxels};
      const int64_t box[9] = {o.first_voxel.x(), o.first_voxel.y(), o.first_voxel.z(), o.bb_min.x(), o.bb_min.y(), o.bb_min.z(),
                              o.bb_max.x(), o.bb_max.y(), o.bb_max.z()};
      const float c[3] = {o.centroid.x(), o.centroid.y(), o.centroid.z()};
      std::fwrite(head, 4, 2, of);
      std::fwrite(box, 8, 9, of);
      std::fwrite(c, 4, 3, of);
    }
    std::fclose(of);
    const ks_objects_stats& os = hip->lastObjectsStats();
    std::printf("adapter_demo: extractObjects %.3f ms, %u objects of %llu components, %llu of %llu surface voxels in objects\n", ms, n_objects,
                (unsigned long long)os.components, (unsigned long long)os.voxels_in_objects, (unsigned long long)os.voxels_surface);
  }

  // KS_DEMO_ALIGN=<file>: the LAST frame's pose, moved by (0.03, -0.02, 0.025) m and turned by 1.5 degrees about
  // (1, 2, -1) / sqrt(6) in the world frame, refined against the map with that frame's cloud on the device without any layer
  // sync (alignPointCloud, default options), written as { f32 T_in[7]; f32 T_out[7]; ks_align_stats (48 bytes) }
  if (const char* align_path = std::getenv("KS_DEMO_ALIGN")) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip || n_frames == 0) return 8;
    const double half = 0.5 * 1.5 * 3.14159265358979323846 / 180.0, s6 = std::sin(half) / std::sqrt(6.0);
    const double dq[4] = {std::cos(half), s6, 2.0 * s6, -s6}, q[4] = {last_T[0], last_T[1], last_T[2], last_T[3]};
    const float T_in[7] = {(float)(dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2] - dq[3] * q[3]),
                           (float)(dq[0] * q[1] + dq[1] * q[0] + dq[2] * q[3] - dq[3] * q[2]),
                           (float)(dq[0] * q[2] - dq[1] * q[3] + dq[2] * q[0] + dq[3] * q[1]),
                           (float)(dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1] + dq[3] * q[0]),
                           last_T[4] + 0.03f, last_T[5] - 0.02f, last_T[6] + 0.025f};
    vxb::Transformation refined;
    const auto t0 = std::chrono::steady_clock::now();
    hip->alignPointCloud(vxb::Transformation(T_in[0], T_in[1], T_in[2], T_in[3], vxb::Point(T_in[4], T_in[5], T_in[6])), last_points,
                         kimera::HipSemanticTsdfIntegrator::AlignOptions(), &refined);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const float T_out[7] = {refined.qw(), refined.qvec().x(), refined.qvec().y(), refined.qvec().z(), refined.getPosition().x(),
                            refined.getPosition().y(), refined.getPosition().z()};
    const ks_align_stats& as = hip->lastAlignStats();
    FILE* af = std::fopen(align_path, "wb");
    if (!af) return 9;
    std::fwrite(T_in, 4, 7, af);
    std::fwrite(T_out, 4, 7, af);
    std::fwrite(&as, sizeof(as), 1, af);
    std::fclose(af);
    std::printf("adapter_demo: alignPointCloud %.3f ms, status %u after %u iterations, %llu of %llu points inliers, rmse %.4f -> %.4f m\n", ms, as.status,
                as.iterations, (unsigned long long)as.inliers_first, (unsigned long long)as.points_used, as.rmse_first, as.rmse_last);
  }

  // KS_DEMO_RENDER=<file>: the map seen from the LAST frame's pose, made on the device without any layer sync (renderView;
  // 128 x 96 pixels, fx = fy = 64, cx = 63.5, cy = 47.5), written as { u32 width, height; f32 T_G_C[7]; f32 K[4];
  // f32 depth[w h]; u8 label[w h]; Color[w h]; Point normal[w h]; u64 pixels_hit, pixels_missed, samples }
  if (const char* render_path = std::getenv("KS_DEMO_RENDER")) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip || n_frames == 0) return 8;
    const uint32_t rw = 128, rh = 96;
    const float K[4] = {64.0f, 64.0f, 63.5f, 47.5f};
    kimera::HipSemanticTsdfIntegrator::RenderedView view;
    const auto t0 = std::chrono::steady_clock::now();
    hip->renderView(vxb::Transformation(last_T[0], last_T[1], last_T[2], last_T[3], vxb::Point(last_T[4], last_T[5], last_T[6])), K[0], K[1],
                    K[2], K[3], rw, rh, kimera::HipSemanticTsdfIntegrator::RenderOptions(), &view);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE* rf = std::fopen(render_path, "wb");
    if (!rf) return 9;
    const ks_render_stats& rs = hip->lastRenderStats();
    const uint64_t counts[3] = {rs.pixels_hit, rs.pixels_missed, rs.samples};
    std::fwrite(&rw, 4, 1, rf);
    std::fwrite(&rh, 4, 1, rf);
    std::fwrite(last_T, 4, 7, rf);
    std::fwrite(K, 4, 4, rf);
    std::fwrite(view.depth.data(), 4, view.depth.size(), rf);
    std::fwrite(view.labels.data(), 1, view.labels.size(), rf);
    std::fwrite(view.colors.data(), sizeof(vxb::Color), view.colors.size(), rf);
    std::fwrite(view.normals.data(), sizeof(vxb::Point), view.normals.size(), rf);
    std::fwrite(counts, 8, 3, rf);
    std::fclose(rf);
    std::printf("adapter_demo: renderView %.3f ms, %u x %u pixels, %llu hit, %.1f samples per pixel\n", ms, rw, rh,
                (unsigned long long)rs.pixels_hit, (double)rs.samples / (double)(rw * rh));
  }

  // ... the blocks of the refresh replace or join the ones kept since the update; the file has the format of KS_DEMO_ESDF
  if (esdf_refresh_path) {
    auto* hip = dynamic_cast<kimera::HipSemanticTsdfIntegrator*>(integrator.get());
    if (!hip) return 8;
    std::vector<EsdfBlock> changed;
    const auto t0 = std::chrono::steady_clock::now();
    hip->refreshEsdf(&changed);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const size_t n_changed = changed.size(), n_before = esdf_kept.size();
    for (auto& eb : changed) esdf_kept[{eb.index.x(), eb.index.y(), eb.index.z()}] = std::move(eb);
    FILE* ef = std::fopen(esdf_refresh_path, "wb");
    if (!ef) return 9;
    const uint32_t n_esdf_blocks = esdf_kept.size(), esdf_vps = tsdf_layer.voxels_per_side();
    std::fwrite(&n_esdf_blocks, 4, 1, ef);
    std::fwrite(&esdf_vps, 4, 1, ef);
    for (const auto& kv : esdf_kept) {
      std::fwrite(kv.first.data(), 4, 3, ef);
      std::fwrite(kv.second.voxels.data(), sizeof(kv.second.voxels[0]), kv.second.voxels.size(), ef);
    }
    std::fclose(ef);
    const ks_esdf_refresh_stats& rs = hip->lastEsdfRefreshStats();
    std::printf("adapter_demo: refreshEsdf %.3f ms, %zu blocks changed, %zu kept from the update, %llu of %llu tiles recomputed (%llu stale)\n", ms,
                n_changed, n_before, (unsigned long long)rs.tiles_recomputed, (unsigned long long)rs.tiles_total, (unsigned long long)rs.tiles_stale);
  }

  vxb::BlockIndexList blocks;
  tsdf_layer.getAllAllocatedBlocks(&blocks);
  std::sort(blocks.begin(), blocks.end(), [](const vxb::BlockIndex& a, const vxb::BlockIndex& b) {
    if (a.x() != b.x()) return a.x() < b.x();
    if (a.y() != b.y()) return a.y() < b.y();
    return a.z() < b.z();
  });
  FILE* out = std::fopen(argv[4], "wb");
  if (!out) return 4;
  const uint32_t nb = blocks.size(), vps = 16;
  std::fwrite(&nb, 4, 1, out);
  std::fwrite(&vps, 4, 1, out);
  size_t updated = 0;
  for (const auto& b : blocks) {
    const int32_t idx[3] = {b.x(), b.y(), b.z()};
    std::fwrite(idx, 4, 3, out);
    auto tb = tsdf_layer.getBlockPtrByIndex(b);
    auto sb = semantic_layer.getBlockPtrByIndex(b);
    if (!sb) return 5;
    updated += tb->updated() && sb->updated();
    for (size_t i = 0; i < tb->num_voxels(); ++i) {
      const vxb::TsdfVoxel& v = tb->getVoxelByLinearIndex(i);
      uint8_t rec[12];
      std::memcpy(rec, &v.distance, 4);
      std::memcpy(rec + 4, &v.weight, 4);
      rec[8] = v.color.r; rec[9] = v.color.g; rec[10] = v.color.b; rec[11] = v.color.a;
      std::fwrite(rec, 1, 12, out);
    }
    for (size_t i = 0; i < sb->num_voxels(); ++i) {
      const kimera::SemanticVoxel& s = sb->getVoxelByLinearIndex(i);
      uint8_t rec[92];
      std::memset(rec, 0, 92);
      rec[0] = s.semantic_label;
      for (int l = 0; l < 21; ++l) {
        const float p = s.semantic_priors[l];
        std::memcpy(rec + 4 + 4 * l, &p, 4);
      }
      rec[88] = s.color.r; rec[89] = s.color.g; rec[90] = s.color.b; rec[91] = s.color.a;
      std::fwrite(rec, 1, 92, out);
    }
  }
  std::fclose(out);
  std::printf("adapter_demo: %u frames, %u blocks (%zu flagged updated)\n", n_frames, nb, updated);
  // what SemanticTsdfServer prints when verbose (voxblox::timing::Timing::Print): the integrator's scopes
  std::printf("timing:\n%s", vxb::timing::Timing::Print().c_str());
  return updated == nb ? 0 : 6;
}
