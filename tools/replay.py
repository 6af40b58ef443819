#!/usr/bin/env python3
"""Offline replay through the MI355X integrator — the role of the reference's kimera_semantics_rosbag executable
(kimera_semantics_ros/src/kimera_semantics_rosbag.cpp:83-141) for the path this repository accelerates: read a ROS1
bag (or generate the synthetic stand-in), compose T_G_C = T_G_B * T_B_C per depth image, integrate depth + labels on
the GPU (ks_integrate_depth), report frames/s and voxel updates/s.  The semantic mesh — what the reference's executable
generates at the end of a bag (:147-167) — is extracted on the device (ks_mesh_update) with --mesh / --mesh-every, and the
batch ESDF it ends with is computed on the device (ks_esdf_update) with --esdf, and kept up to date while frames stream in
(ks_esdf_refresh) with --esdf-every; --render-every writes what the map looks like from the frame's own pose and intrinsics
(ks_render_view: depth, labels, colours, normals) every N frames; --align refines every frame's pose against the map on the
device before the frame is integrated (ks_align_points: what `enable_icp` selects in the reference's launch files, without a layer
sync) and prints the correction; --objects clusters the surface of every label into object instances on the device at the end
of the replay (ks_objects_update) and writes their records, centroids in metres and label names; --max-block-distance M prunes the
map around the sensor position after every frame (ks_remove_distant_blocks: what voxblox::TsdfServer does with
max_block_distance_from_body; completes the frames in flight), so that a long replay runs in a bounded pool; --submap-frames N
maps like a submap mapper: every N frames go into a second context in the frame of their first camera pose, which is then fused
into the map at that pose on the device (ks_fuse_map: resampled under SE(3) and merged) and cleared; --nav-goal X,Y,Z --nav-out
writes the cost-to-go field of the final ESDF to that goal for a robot of --nav-radius, made on the device (ks_nav_update), with the
path from the last camera position; map saving stays on the host side of the drop-in boundary (out of scope).
  python tools/replay.py --synthetic 50 [--method merged] [--mesh out.ply] [--mesh-indexed out.ply] [--mesh-every 5] [--esdf out.npz] [--esdf-every 5] \\
      [--nav-goal 0.5,0,0 --nav-radius 0.3 --nav-out nav.npz [--nav-shorten]] [--render-every 10 --render-out views/] [--align --align-iterations 10 --align-dof 0x3c] [--objects out.npz] [--frontiers out.npz] [--rooms out.npz] [--view-gain out.npz] \\
      [--max-block-distance 3.0] [--submap-frames 10]
  python tools/replay.py --bag demo.bag --depth-topic /tesse/depth --semantic-topic /tesse/segmentation \\
      --camera-info-topic /tesse/left_cam/camera_info --sensor-frame left_cam --label-csv cfg/tesse_multiscene_office1_segmentation_mapping.csv"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kimera_semantics_amd import binding as B  # noqa: E402
from kimera_semantics_amd import frame_source as FS  # noqa: E402
from kimera_semantics_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bag")
    ap.add_argument("--synthetic", type=int, default=0, help="number of frames of the synthetic stand-in")
    ap.add_argument("--method", default="fast", choices=["fast", "merged"])
    ap.add_argument("--depth-topic", default="/depth")
    ap.add_argument("--semantic-topic", default="/semantic")
    ap.add_argument("--camera-info-topic", default="/camera_info")
    ap.add_argument("--sensor-frame", default="left_cam")
    ap.add_argument("--base-link-frame", default="base_link_gt")
    ap.add_argument("--world-frame", default="world")
    ap.add_argument("--label-csv", help="the reference's label CSV (name,red,green,blue,alpha,id); default: the synthetic palette")
    ap.add_argument("--voxel-size", type=float, default=0.05)
    ap.add_argument("--pipeline-frames", type=int, default=4)
    ap.add_argument("--mesh", metavar="OUT.ply", help="extract the semantic mesh at the end of the replay and write it (binary PLY with a label property)")
    ap.add_argument("--mesh-indexed", metavar="OUT.ply", help="write the mesh with SHARED vertices (ks_mesh_index on the stored mesh: faces reference the "
                    "vertices, smooth normals, label and object_id vertex properties; object ids where --objects has made objects)")
    ap.add_argument("--mesh-every", type=int, default=0, metavar="N", help="refresh the mesh on the device (only_stale) every N frames")
    ap.add_argument("--esdf", metavar="OUT.npz", help="compute the batch ESDF with nearest-surface labels at the end of the replay and write it "
                    "(block_indices (N, 3), distance / flags / label (N, vps^3) in host block layout, voxel_size, voxels_per_side)")
    ap.add_argument("--esdf-every", type=int, default=0, metavar="N", help="keep an ESDF up to date on the device: ks_esdf_update at the first tick, "
                    "ks_esdf_refresh every N frames after it (with --esdf the file holds the refreshed ESDF)")
    ap.add_argument("--esdf-slice", metavar="OUT.npz", help="write distance, status and label images of the final ESDF over the map's bounding box "
                    "at z = --slice-level, one pixel per voxel, made on the device (ks_esdf_slice: trilinear, NaN where unknown)")
    ap.add_argument("--slice-level", type=float, default=0.0, metavar="Z", help="the reference's slice_level")
    ap.add_argument("--esdf-max-distance", type=float, default=2.0, metavar="M")
    ap.add_argument("--esdf-min-distance", type=float, default=0.2, metavar="M")
    ap.add_argument("--nav-goal", metavar="X,Y,Z", help="with --nav-out: the goal of the navigation field, a world point in metres")
    ap.add_argument("--nav-radius", type=float, default=0.3, metavar="R", help="the robot radius the field is made for")
    ap.add_argument("--nav-shorten", action="store_true", help="with --nav-out: also pull that path taut by line of sight over the ESDF on the device "
                    "(ks_path_shorten, the radius of --nav-radius) and write both path sets (path_short, path_short_status, path_short_length_m, "
                    "path_short_min_clearance_m beside path)")
    ap.add_argument("--nav-out", metavar="OUT.npz", help="compute the cost-to-go field of the final ESDF to --nav-goal on the device (ks_nav_update) and "
                    "write it per block with the path from the last camera position (ks_nav_paths); needs --esdf, --esdf-every or --esdf-slice")
    ap.add_argument("--render-every", type=int, default=0, metavar="N", help="render the map on the device from the frame's own pose and intrinsics "
                    "every N frames (ks_render_view; completes the frames in flight)")
    ap.add_argument("--render-out", metavar="DIR", help="where --render-every writes view_<frame>.npz (depth, labels, rgba, normals, T_G_C, K)")
    ap.add_argument("--render-max-range", type=float, default=10.0, metavar="M")
    ap.add_argument("--align", action="store_true", help="refine every frame's pose against the map on the device before integrating it "
                    "(ks_align_points; skipped while the map is empty; completes the frames in flight)")
    ap.add_argument("--align-iterations", type=int, default=10, metavar="N", help="the reference's icp_iterations")
    ap.add_argument("--align-dof", type=lambda v: int(v, 0), default=0x3f, metavar="MASK", help="bits 0-2 rotation about world x, y, z, bits 3-5 "
                    "translation; 0x3c = yaw and translation")
    ap.add_argument("--align-stride", type=int, default=1, metavar="N", help="use every N-th pixel")
    ap.add_argument("--objects", metavar="OUT.npz", help="cluster the surface voxels of every label into object instances at the end of the replay and "
                    "write them (records (n,) of 72 bytes ascending by first_voxel, centroids_m (n, 3), label_names (n,), voxel_size)")
    ap.add_argument("--objects-min-voxels", type=int, default=8, metavar="N")
    ap.add_argument("--frontiers", metavar="OUT.npz", help="extract the exploration frontiers of the final ESDF on the device (ks_frontiers_update) for a "
                    "robot of --nav-radius and write them (records (n,) of 88 bytes ascending by first_voxel, centroids_m, targets_m, stats, "
                    "block_indices and the per-block ids); needs --esdf; with --nav-goal the records carry the cost-to-go from that goal")
    ap.add_argument("--frontiers-min-voxels", type=int, default=8, metavar="N")
    ap.add_argument("--rooms", metavar="OUT.npz", help="segment the final ESDF into rooms on the device (ks_rooms_update) and write them (records (n,) of "
                    "96 bytes ascending by first_voxel, links (m,) of 32 bytes, centroids_m, centres_m, room_of_object (with --objects), stats, "
                    "block_indices and the per-block room and cost planes); needs --esdf")
    ap.add_argument("--rooms-core-distance", type=float, default=0.5, metavar="M")
    ap.add_argument("--rooms-min-core-voxels", type=int, default=64, metavar="N")
    ap.add_argument("--view-gain", metavar="OUT.npz", help="score candidate camera poses by the unknown voxels of the final ESDF they would see, on the "
                    "device (ks_view_gain): the centres of the frontiers' nav_voxel (the frontiers as --frontiers makes them), each at 8 yaws, "
                    "--view-gain-size rays of a 90-degree image, --view-gain-range metres; writes poses (n, 7), records (n,) of 32 bytes, stats; "
                    "needs --esdf")
    ap.add_argument("--view-gain-size", default="32x24", metavar="WxH")
    ap.add_argument("--view-gain-range", type=float, default=5.0, metavar="M")
    ap.add_argument("--max-block-distance", type=float, default=None, metavar="M", help="after every frame remove the blocks whose origin is further "
                    "than M metres from the sensor position (ks_remove_distant_blocks; completes the frames in flight)")
    ap.add_argument("--submap-frames", type=int, default=0, metavar="N", help="integrate every N frames into a second context, in the frame of "
                    "their first camera pose, and fuse it into the map at that pose (ks_fuse_map), then clear it")
    ap.add_argument("--submap-min-weight", type=float, default=1e-4, metavar="W")
    a = ap.parse_args()
    if a.render_every and not a.render_out:
        ap.error("--render-every needs --render-out")
    if bool(a.nav_out) != bool(a.nav_goal):
        ap.error("--nav-out and --nav-goal go together")
    if a.nav_shorten and not a.nav_out:
        ap.error("--nav-shorten goes with --nav-out")
    if a.nav_out and not (a.esdf or a.esdf_every or a.esdf_slice):
        ap.error("--nav-out plans over the stored ESDF: give --esdf, --esdf-every or --esdf-slice as well")
    if a.frontiers and not a.esdf:
        ap.error("--frontiers reads the stored ESDF: give --esdf as well")
    if a.rooms and not a.esdf:
        ap.error("--rooms reads the stored ESDF: give --esdf as well")
    if a.view_gain and not a.esdf:
        ap.error("--view-gain reads the stored ESDF: give --esdf as well")
    if a.nav_goal:
        try:
            nav_goal = np.array([float(v) for v in a.nav_goal.split(",")], np.float32)
            assert nav_goal.shape == (3,)
        except (ValueError, AssertionError):
            ap.error("--nav-goal takes X,Y,Z")
    if a.bag:
        seq = FS.read_rosbag(a.bag, a.depth_topic, a.semantic_topic, a.camera_info_topic, a.sensor_frame, a.base_link_frame, a.world_frame)
    else:
        seq = FS.synthetic_sequence(a.synthetic or 20)
    lut = synth.default_label_colors()
    names = {}
    if a.label_csv:
        import csv
        lut = np.zeros((256, 4), np.uint8)
        for row in csv.reader(open(a.label_csv)):
            try:
                lut[int(row[5])] = [int(row[1]), int(row[2]), int(row[3]), int(row[4])]
                names.setdefault(int(row[5]), row[0])
            except (ValueError, IndexError):
                continue
        lut[0] = [255, 255, 255, 255]
    h0, w0 = seq.frames[0].depth.shape
    cfg = B.default_config(method=0 if a.method == "fast" else 1, voxel_size=a.voxel_size, truncation_distance=4 * a.voxel_size,
                           semantic_measurement_probability=0.8, dynamic_labels=[20], label_rgba=lut, max_points=h0 * w0,
                           pipeline_frames=a.pipeline_frames)
    integ = B.HipIntegrator(cfg)
    integ.set_color_to_label(lut[:21], np.arange(21, dtype=np.uint8))
    upd = 0

    class Submapper:
        """What FS.replay integrates into with --submap-frames: a second context that holds the current submap, in the frame of the
        submap's first camera pose (T_G_S); after N frames it is fused into the map at T_G_S and emptied."""

        def __init__(self):
            self.ctx = B.HipIntegrator(cfg)
            self.ctx.set_color_to_label(lut[:21], np.arange(21, dtype=np.uint8))
            self.T_G_S, self.n, self.fused, self.seconds, self.updates = None, 0, [], 0.0, 0

        def integrate_depth(self, T_G_C, depth, K, **kw):
            if self.n == a.submap_frames:
                self.fuse()
            if self.T_G_S is None:
                self.T_G_S = np.asarray(T_G_C, np.float32).copy()
            self.n += 1
            return self.ctx.integrate_depth(FS.compose(FS.inverse(self.T_G_S), T_G_C), depth, K, **kw)

        def fuse(self):
            if self.T_G_S is None:
                return
            t1 = time.perf_counter()
            self.updates += self.ctx.flush().n_voxel_updates
            self.fused.append(integ.fuse(self.ctx, self.T_G_S, min_weight=a.submap_min_weight))
            self.ctx.clear()
            self.seconds += time.perf_counter() - t1
            self.T_G_S, self.n = None, 0

    sub = Submapper() if a.submap_frames > 0 else None

    refresh_s, refreshes, n_seen = 0.0, [], 0
    esdf_s, esdf_ticks = 0.0, []
    esdf_cfg = dict(min_distance_m=a.esdf_min_distance, max_distance_m=a.esdf_max_distance)
    render_s, renders = 0.0, []
    if a.render_every:
        os.makedirs(a.render_out, exist_ok=True)

    prune_s, prunes = 0.0, []
    last_position = None

    def acc(fr, T, st):
        nonlocal upd, refresh_s, n_seen, esdf_s, render_s, prune_s, last_position
        upd += st.n_voxel_updates
        last_position = np.asarray(T, np.float32)[4:7].copy()
        n_seen += 1
        if a.max_block_distance is not None:   # first: what the later ticks of this frame see is the pruned map
            t1 = time.perf_counter()
            prunes.append(integ.remove_distant(np.asarray(T, np.float32)[4:7], a.max_block_distance))
            prune_s += time.perf_counter() - t1
        if a.esdf_every and n_seen % a.esdf_every == 0:
            t1 = time.perf_counter()
            if esdf_ticks:
                es = integ.esdf_refresh()
            else:
                es = dict(integ.esdf_update(**esdf_cfg), tiles_recomputed=None)
            esdf_s += time.perf_counter() - t1
            esdf_ticks.append(es)
        if a.render_every and n_seen % a.render_every == 0:
            hh, ww = fr.depth.shape
            t1 = time.perf_counter()
            depth, labels, rgba, normals, rs = integ.render(T, fr.K, ww, hh, max_range_m=a.render_max_range)
            render_s += time.perf_counter() - t1
            renders.append(rs)
            np.savez_compressed(os.path.join(a.render_out, "view_%06d.npz" % n_seen), depth=depth, labels=labels, rgba=rgba, normals=normals,
                                T_G_C=np.asarray(T, np.float32), K=np.asarray(fr.K, np.float32))
        if a.mesh_every and n_seen % a.mesh_every == 0:
            t1 = time.perf_counter()
            m = integ.mesh(only_stale=True)        # (completes the frames in flight, like every query)
            refresh_s += time.perf_counter() - t1
            refreshes.append((m.stats["blocks_meshed"], m.stats["blocks_total"], m.n_triangles))
    align_s, aligned = 0.0, []

    def refine(fr, T):
        nonlocal align_s
        if len(integ.block_indices()) == 0:     # nothing to align against yet
            return T
        xyz = synth.backproject(np.asarray(fr.depth, np.float32), fr.K).reshape(-1, 3)
        t1 = time.perf_counter()
        T_out, st = integ.align(T, xyz, max_iterations=a.align_iterations, dof_mask=a.align_dof, point_stride=a.align_stride)
        align_s += time.perf_counter() - t1
        aligned.append(st)
        dt_m = float(np.linalg.norm(T_out[4:].astype(np.float64) - np.asarray(T, np.float64)[4:]))
        dot = abs(float(np.dot(T_out[:4].astype(np.float64), np.asarray(T, np.float64)[:4]))) / float(np.linalg.norm(np.asarray(T, np.float64)[:4]))
        print(f"frame {len(aligned)}: pose corrected by {dt_m * 1e3:.2f} mm, {np.degrees(2 * np.arccos(min(dot, 1.0))):.4f} deg; status {st['status']} after "
              f"{st['iterations']} iterations, {st['inliers_first']} of {st['points_used']} points inliers, rmse {st['rmse_first']:.4f} -> {st['rmse_last']:.4f} m")
        return T_out

    t0 = time.perf_counter()
    out = FS.replay(seq, sub or integ, use_label_img=not a.bag, on_frame=acc, refine=refine if a.align else None)
    if sub:
        sub.fuse()
        upd += sub.updates
    upd += integ.flush().n_voxel_updates
    integ.synchronize()
    dt = time.perf_counter() - t0
    print(f"{out['integrated']} frames integrated ({out['skipped_no_tf']} skipped: no tf) in {dt:.3f} s: "
          f"{out['integrated'] / dt:.1f} frames/s incl. H2D of the images, {upd / dt / 1e6:.1f} M voxel updates/s, "
          f"{len(integ.block_indices())} blocks")
    if sub and sub.fused:
        print(f"{len(sub.fused)} submaps of {a.submap_frames} frames fused (incl. their flush and clear) in {sub.seconds * 1e3:.1f} ms of the above: "
              f"{sub.seconds / len(sub.fused) * 1e3:.2f} ms each; {sum(f['voxels_fused'] for f in sub.fused)} voxels fused into "
              f"{sum(f['tiles_touched'] for f in sub.fused)} tiles ({sum(f['tiles_allocated'] for f in sub.fused)} new) from "
              f"{sum(f['tiles_source'] for f in sub.fused)} submap tiles, work space at most {max(f['workspace_bytes'] for f in sub.fused) / 2 ** 20:.1f} MiB")
        sub.ctx.close()
    if prunes:
        print(f"pruned after every frame beyond {a.max_block_distance} m in {prune_s * 1e3:.1f} ms of the above: {prune_s / len(prunes) * 1e3:.3f} ms each; "
              f"{sum(p['blocks_removed'] for p in prunes)} blocks removed, {sum(p['tiles_moved'] for p in prunes)} tiles moved, at most "
              f"{max(p['tiles_resident'] for p in prunes)} tiles resident afterwards, pool of {prunes[-1]['pool_capacity_tiles']} tiles")
    if refreshes:
        print(f"{len(refreshes)} mesh refreshes (only_stale, incl. the download) in {refresh_s * 1e3:.1f} ms of the above: "
              f"{refresh_s / len(refreshes) * 1e3:.2f} ms each; last: {refreshes[-1][0]} of {refreshes[-1][1]} blocks re-meshed, "
              f"{refreshes[-1][2]} triangles")
    if len(esdf_ticks) > 1:
        last = esdf_ticks[-1]
        print(f"1 ESDF update and {len(esdf_ticks) - 1} refreshes in {esdf_s * 1e3:.1f} ms of the above; last refresh: {last['tiles_recomputed']} of "
              f"{last['tiles_total']} tiles recomputed ({last['tiles_stale']} stale), work space {last['workspace_bytes'] / 2 ** 20:.1f} MiB")
    if aligned:
        print(f"{len(aligned)} poses refined (incl. the upload of the cloud) in {align_s * 1e3:.1f} ms of the above: {align_s / len(aligned) * 1e3:.2f} ms each; "
              f"{sum(s['status'] == B.KS_ALIGN_CONVERGED for s in aligned)} converged")
    if renders:
        last = renders[-1]
        print(f"{len(renders)} views rendered (incl. the download of the four images) in {render_s * 1e3:.1f} ms of the above: "
              f"{render_s / len(renders) * 1e3:.2f} ms each; last: {last['pixels_hit']} of {last['pixels_hit'] + last['pixels_missed']} pixels hit, "
              f"{last['samples'] / (last['pixels_hit'] + last['pixels_missed']):.1f} samples per pixel -> {a.render_out}")
    if a.mesh:
        from kimera_semantics_amd.mesh import write_ply
        t1 = time.perf_counter()
        m = integ.mesh(only_stale=bool(refreshes))
        t_mesh = time.perf_counter() - t1
        write_ply(a.mesh, m)
        print(f"mesh: {m.n_triangles} triangles in {len(m.blocks)} blocks, labels {sorted(set(m.labels.tolist()))}, "
              f"{t_mesh * 1e3:.2f} ms (extraction + download) -> {a.mesh}")
    if a.esdf:
        t1 = time.perf_counter()
        if esdf_ticks:   # the stored ESDF brought up to date with the last frames
            st = integ.esdf_refresh()
            idx = integ.block_indices()
            rec = integ.esdf_blocks(idx)
        else:
            idx, rec, st = integ.esdf(**esdf_cfg)
        t_esdf = time.perf_counter() - t1
        np.savez_compressed(a.esdf, block_indices=idx, distance=rec["distance"], flags=rec["flags"], label=rec["label"],
                            voxel_size=np.float32(a.voxel_size), voxels_per_side=np.int32(integ.vps))
        how = f"{st['tiles_recomputed']} of {st['tiles_total']} tiles recomputed" if esdf_ticks else f"box {st['box_voxels']}"
        print(f"esdf: {st['voxels_observed']} observed voxels ({st['voxels_fixed']} in the band, {st['voxels_clamped']} at +-{a.esdf_max_distance} m), "
              f"{how}, work space {st['workspace_bytes'] / 2 ** 20:.1f} MiB, {t_esdf * 1e3:.2f} ms ({'refresh' if esdf_ticks else 'update'} + download) -> {a.esdf}")
    if a.esdf_slice:
        if a.esdf or esdf_ticks:   # an ESDF is stored: bring it up to date (nothing is recomputed when it is)
            integ.esdf_refresh()
        else:
            integ.esdf_update(**esdf_cfg)
        idx = integ.block_indices()
        side = integ.vps * a.voxel_size
        lo, hi = idx.min(axis=0) * side, (idx.max(axis=0) + 1) * side
        w, h = int(round((hi[0] - lo[0]) / a.voxel_size)), int(round((hi[1] - lo[1]) / a.voxel_size))
        origin = [lo[0] + 0.5 * a.voxel_size, lo[1] + 0.5 * a.voxel_size, a.slice_level]   # pixel (i, j) at the centre of voxel column (i, j)
        t1 = time.perf_counter()
        img = integ.esdf_slice(origin, [a.voxel_size, 0, 0], [0, a.voxel_size, 0], w, h, outputs=("distance", "status", "label"))
        t_slice = time.perf_counter() - t1
        np.savez_compressed(a.esdf_slice, distance=img["distance"], status=img["status"], label=img["label"], origin=np.float32(origin),
                            voxel_size=np.float32(a.voxel_size), slice_level=np.float32(a.slice_level))
        st = img["stats"]
        print(f"esdf slice at z = {a.slice_level} m: {w} x {h} pixels, {st['points_interpolated']} interpolated, {st['points_nearest']} nearest, "
              f"{st['points_unknown']} unknown, {t_slice * 1e3:.2f} ms (slice + download) -> {a.esdf_slice}")
    if a.nav_out:   # (after the ESDF outputs: the store is up to date)
        if not (a.esdf or a.esdf_slice):
            integ.esdf_refresh()   # (--esdf-every alone: the last ticks' frames)
        t1 = time.perf_counter()
        st = integ.nav_update(nav_goal[None], radius_m=a.nav_radius)
        idx = integ.block_indices()
        field = integ.nav_blocks(idx)
        path = integ.nav_paths(last_position[None], 65536, outputs=("status", "cost", "n_waypoints", "waypoints"))
        t_nav = time.perf_counter() - t1
        n_wp = int(path["n_waypoints"][0])
        short = {}
        if a.nav_shorten:
            t1 = time.perf_counter()
            taut = integ.shorten_paths(path["waypoints"][:, :max(n_wp, 1)], path["n_waypoints"], radius_m=a.nav_radius)
            t_short = time.perf_counter() - t1
            n_short = int(taut["n_waypoints"][0])
            short = dict(path_short=taut["waypoints"][0, :n_short], path_short_status=taut["status"][0], path_short_length_m=taut["length"][0],
                         path_short_min_clearance_m=taut["min_clearance"][0])
        np.savez_compressed(a.nav_out, block_indices=idx, cost=field, goal=nav_goal, radius_m=np.float32(a.nav_radius), start=last_position,
                            path_status=path["status"][0], path_cost=path["cost"][0], path=path["waypoints"][0, :n_wp],
                            voxel_size=np.float32(a.voxel_size), voxels_per_side=np.int32(integ.vps), **short)
        what = {B.KS_NAV_PATH_REACHED: "reaches the goal", B.KS_NAV_PATH_UNREACHABLE: "cannot reach the goal", B.KS_NAV_PATH_BLOCKED: "starts in a voxel "
                "that is not traversable", B.KS_NAV_PATH_TRUNCATED: "was cut at 65536 waypoints"}.get(int(path["status"][0]), "is invalid")
        print(f"nav: {st['voxels_reached']} of {st['voxels_traversable']} traversable voxels reached for radius {a.nav_radius} m ({st['goals_used']} of 1 goals "
              f"usable), largest cost {st['largest_cost']}, {st['rounds']} rounds, {st['tile_relaxations']} tile relaxations; the path from the last camera "
              f"position {what}: {n_wp} waypoints, about {int(path['cost'][0]) * a.voxel_size / 10 if n_wp else 0:.2f} m; {t_nav * 1e3:.2f} ms "
              f"(field + download + path) -> {a.nav_out}")
        if a.nav_shorten:
            what = {B.KS_SHORTEN_OK: "every segment verified", B.KS_SHORTEN_UNVERIFIED: "with segments no sweep verified"}.get(int(taut["status"][0]), "invalid: no path")
            print(f"nav shorten: {n_wp} -> {n_short} waypoints ({what}), {float(taut['length'][0]):.2f} m, smallest clearance "
                  f"{float(taut['min_clearance'][0]):.3f} m, {taut['stats']['sweeps']} sweeps of {taut['stats']['samples']} samples; {t_short * 1e3:.2f} ms")
    if a.frontiers:   # (after --nav-out: a stored field fills the join)
        t1 = time.perf_counter()
        rec, st = integ.frontiers(radius_m=a.nav_radius, min_voxels=a.frontiers_min_voxels)
        idx = integ.block_indices()
        ids = integ.frontier_ids(idx)
        t_fr = time.perf_counter() - t1
        np.savez_compressed(a.frontiers, records=rec, centroids_m=B.frontier_centroids(rec, integ.cfg.voxel_size),
                            targets_m=B.frontier_targets(rec, integ.cfg.voxel_size), stats_names=np.array(list(st)), stats=np.array(list(st.values()), np.uint64),
                            block_indices=idx, ids=ids, radius_m=np.float32(a.nav_radius), voxel_size=np.float32(a.voxel_size), voxels_per_side=np.int32(integ.vps))
        reached = int((rec["nav_cost"] <= B.KS_NAV_MAX_COST).sum())
        print(f"frontiers: {st['frontiers']} frontiers of {st['components']} components over {st['voxels_frontier']} frontier voxels "
              f"({st['voxels_in_frontiers']} in frontiers, the largest {st['largest_frontier_voxels']}), {st['unknown_faces']} unknown faces, "
              f"{reached} reached by the field" + ("" if st["nav_field_used"] else " (no field stored: give --nav-goal)") +
              f", work space {st['workspace_bytes'] / 2 ** 20:.1f} MiB, {t_fr * 1e3:.2f} ms (update + records + ids) -> {a.frontiers}")
    if a.rooms:
        if a.objects:   # stored objects are joined to their rooms (the --objects step below makes the same ones again)
            integ.objects(min_voxels=a.objects_min_voxels)
        t1 = time.perf_counter()
        rec, links, st = integ.rooms(core_distance_m=a.rooms_core_distance, min_core_voxels=a.rooms_min_core_voxels)
        idx = integ.block_indices()
        t_rm = time.perf_counter() - t1
        np.savez_compressed(a.rooms, records=rec, links=links, centroids_m=B.room_centroids(rec, integ.cfg.voxel_size),
                            centres_m=B.room_centres(rec, integ.cfg.voxel_size), room_of_object=integ.room_objects(), stats_names=np.array(list(st)),
                            stats=np.array(list(st.values()), np.uint64), block_indices=idx, room_ids=integ.room_ids(idx), room_costs=integ.room_costs(idx),
                            core_distance_m=np.float32(a.rooms_core_distance), voxel_size=np.float32(a.voxel_size), voxels_per_side=np.int32(integ.vps))
        print(f"rooms: {st['rooms']} rooms of {st['components']} core components, {st['links']} links over {st['contacts']} contacts, "
              f"{st['voxels_assigned']} of {st['voxels_free']} free voxels assigned (the largest room {st['largest_room_voxels']}), "
              f"{st['objects_joined']} of {st['objects_seen']} objects joined, {st['rounds']} rounds, work space {st['workspace_bytes'] / 2 ** 20:.1f} MiB, "
              f"{t_rm * 1e3:.2f} ms (update + records + links) -> {a.rooms}")
    if a.view_gain:   # (after --frontiers: the candidates stand where the frontiers are best reached)
        vw, vh = (int(v) for v in a.view_gain_size.lower().split("x"))
        frec, _ = integ.frontiers(radius_m=a.nav_radius, min_voxels=a.frontiers_min_voxels)
        poses = B.view_gain_yaw_poses(B.frontier_targets(frec, integ.cfg.voxel_size), 8)
        vK = (0.5 * vw, 0.5 * vw, (vw - 1) / 2, (vh - 1) / 2)
        t1 = time.perf_counter()
        rec, st = integ.view_gain(poses, vK, vw, vh, max_range_m=a.view_gain_range)
        t_vg = time.perf_counter() - t1
        np.savez_compressed(a.view_gain, poses=poses, records=rec, stats_names=np.array(list(st)), stats=np.array(list(st.values()), np.uint64),
                            K=np.array(vK, np.float32), width=np.int32(vw), height=np.int32(vh), max_range_m=np.float32(a.view_gain_range),
                            voxel_size=np.float32(a.voxel_size))
        best = int(np.argmax(rec["unknown_voxels"])) if len(rec) else -1
        print(f"view gain: {len(poses)} candidate views at {len(frec)} frontiers, {st['samples'] / max(len(poses), 1):.0f} samples per view, "
              f"{st['views_in_lds']} with their visited bitmap in LDS" +
              (f", the best (view {best}, at {poses[best, 4:7].round(2).tolist()}) sees {int(rec['unknown_voxels'][best])} unknown voxels" if best >= 0 else "") +
              f", work space {st['workspace_bytes'] / 2 ** 20:.1f} MiB, {t_vg * 1e3:.2f} ms -> {a.view_gain}")
    if a.objects:
        t1 = time.perf_counter()
        rec, st = integ.objects(min_voxels=a.objects_min_voxels)
        t_obj = time.perf_counter() - t1
        label_names = np.array([names.get(int(l), "label_%d" % int(l)) for l in rec["label"]])
        np.savez_compressed(a.objects, records=rec, centroids_m=B.object_centroids(rec, integ.cfg.voxel_size), label_names=label_names,
                            voxel_size=np.float32(a.voxel_size))
        print(f"objects: {st['objects']} objects of {st['components']} components over {st['voxels_surface']} surface voxels "
              f"({st['voxels_in_objects']} in objects, the largest {st['largest_object_voxels']}), labels {sorted(set(rec['label'].tolist()))}, "
              f"work space {st['workspace_bytes'] / 2 ** 20:.1f} MiB, {t_obj * 1e3:.2f} ms (update + download) -> {a.objects}")
    if a.mesh_indexed:   # (after --objects, so that the vertices carry their ids)
        from kimera_semantics_amd.mesh import write_ply
        integ.mesh(only_stale=True)        # the stored mesh up to date (everything, if nothing has meshed yet)
        t1 = time.perf_counter()
        im = integ.mesh_index()
        t_index = time.perf_counter() - t1
        write_ply(a.mesh_indexed, im)
        print(f"indexed mesh: {im.n_vertices} vertices for {im.stats['corners']} corners ({im.n_triangles} triangles), at most "
              f"{im.stats['max_corners_per_vertex']} corners on a vertex, {int((im.object_ids != B.KS_OBJECT_NONE).sum())} vertices in objects, "
              f"{t_index * 1e3:.2f} ms (index + download) -> {a.mesh_indexed}")


if __name__ == "__main__":
    main()
