#!/usr/bin/env python3
"""TSDF volume integration (UniformTSDFVolume on its own handle) on the MI355X: what a call costs, how much of it is the
kernel, and what applying several frames per pass over the volume buys.

  (1) 64 frames of 640 x 480 uint16 (the analytic scene of examples/teaser_python_tsdf.py, 16 poses four times over)
      into R = 256 and R = 512, without colour and with RGB8, in ONE call (passes of 8 frames) and as 64 calls (passes
      of one frame); the two volumes must hold the same bits;
  (2) extract_point_cloud (with normals) and extract_voxel_point_cloud from each of those volumes;
  (3) the numpy restatement (tests/tsdf_reference.py) at R = 32 on 8 frames of 160 x 120, for context only.

Call times are a host clock around a Python call that ends in a device synchronise, after `--warmup` untimed calls:
median, minimum and maximum of `--reps` (at least nine).  An integration call includes the host's checks, the packing of
the rows into page-locked memory, the upload, the launches and the synchronisation.  The volume keeps accumulating over
the timed calls: the voxels a frame touches do not depend on what the volume holds, so every call does the same work.

Kernel time comes from a run of its own: `--profile-workload` runs the calls of (1) and (2) at one setting and writes
nothing; `rocprofv3 --kernel-trace --stats` is pointed at it, and its kernel_stats.csv is kept beside the JSON.  The
bytes the integration kernel moves per pass -- every touched voxel read and written once, plus the images read once --
follow from `touched_voxels_per_pass` in the JSON (counted at R <= 256 by integrating each chunk into an emptied volume
and downloading the weights); over the kernel's time they give the share of the 8 TB/s HBM peak that
profiles/tsdf/README.md works out.  Needs an MI355X: there is no CPU path.

    python scripts/bench_tsdf.py --reps 9 --warmup 1 --out profiles/tsdf/bench_tsdf.json

`--mesh` measures the triangle mesh instead (profiles/tsdf_mesh/): on the same 64-frame scene at every size of `--sizes`,
with RGB8 colour, extract_triangle_mesh (a count call and a fill call, as the Python method makes them) with and without
vertex normals beside the handle's own extract_point_cloud, and the Python restatement of the mesh
(tests/tsdf_mesh_reference.py) on the volume downloaded at R = 64, which must equal the device's mesh.
`--profile-workload mesh` runs three mesh extractions for rocprofv3.

    python scripts/bench_tsdf.py --mesh --reps 9 --warmup 1 --out profiles/tsdf_mesh/bench_tsdf_mesh.json

`--ray-cast` measures the ray cast instead (profiles/tsdf_raycast/): on the same 64-frame scene at every size of
`--sizes`, with RGB8 colour, one 640 x 480 view at the first pose with all maps and with the depth alone, 16 views (the
16 poses) in one call against 16 calls, and -- the only route to a model depth image without the ray cast --
extract_point_cloud followed by project_to_depth_image on the same volume and pose, with the share of the image each
route fills.  The steps every ray takes are counted by the numpy restatement (tests/tsdf_raycast_reference.py) on the
volume downloaded at R = 64, which must equal the device's maps.  `--profile-workload ray_cast` runs three single-view
and three 16-view calls for rocprofv3.

    python scripts/bench_tsdf.py --ray-cast --reps 9 --warmup 1 --out profiles/tsdf_raycast/bench_tsdf_raycast.json

`--scalable` measures the scalable volume instead (profiles/tsdf_scalable/): the same 64 frames into a ScalableTSDFVolume
with the voxels of every size of `--sizes`, without and with RGB8 colour: the time of one call of 64 frames and of 64
calls, each into an emptied volume (every block is opened again) and into a volume whose blocks are open, per call and
per frame and split by the library's own clock into touch pass, directory merge and integration; the extractions; the
blocks opened and the device bytes they hold beside the dense cube's; and the dense volume's times on the same frames in
the same process, measured in alternation with the scalable ones (that is the comparison: the dense path is unchanged).

    python scripts/bench_tsdf.py --scalable --sizes 512 --reps 9 --warmup 1 --out profiles/tsdf_scalable/bench_tsdf_scalable.json

`--scalable --ray-cast` measures the ray cast of the scalable volume (profiles/tsdf_scalable_raycast/): the 64 RGB8 frames
into a ScalableTSDFVolume with the voxels of every size of `--sizes` and, in the same process, into the dense volume; one
640 x 480 view at the first pose with all maps and with the depth alone and 16 views in one call on both, measured in
alternation; extract_point_cloud(normals=False) + project_to_depth_image on the scalable volume; and, from the trace of
the numpy restatement (tests/stsdf_raycast_reference.py) on the very volume that was timed (the first of `--sizes`, all 64
frames, downloaded) and a 160 x 120 view, which must equal the device's maps: the steps per ray, the share of them in blocks that are not open and
the directory searches (block changes) per ray.  `--profile-workload scalable_ray_cast` runs three single-view and three
16-view calls on both volumes for rocprofv3.

    python scripts/bench_tsdf.py --scalable --ray-cast --sizes 512 --reps 9 --warmup 1 --out profiles/tsdf_scalable_raycast/bench_tsdf_scalable_raycast.json

`--scalable --mesh` measures the triangle mesh of the scalable volume (profiles/tsdf_scalable_mesh/): the 64 RGB8 frames
into a ScalableTSDFVolume with the voxels of every size of `--sizes` and, in the same process, into the dense volume;
extract_mesh (a count call and a fill call) with and without vertex normals, the counts-only call and the scalable
extract_point_cloud beside the dense extract_triangle_mesh on the same frames, measured in alternation; and the Python
restatement of the mesh (tests/stsdf_mesh_reference.py) on the blocks downloaded at the voxels of R = 64, which must
equal the device's mesh.  `--profile-workload scalable_mesh` runs three mesh extractions with normals on both volumes
for rocprofv3.

    python scripts/bench_tsdf.py --scalable --mesh --sizes 512 --reps 9 --warmup 1 --out profiles/tsdf_scalable_mesh/bench_tsdf_scalable_mesh.json"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
tp = importlib.import_module("teaser-plusplus_amd")
ex = importlib.import_module("teaser_python_tsdf")

W, H, FRAMES, POSES, CHUNK = 640, 480, 64, 16, 8
HBM_PEAK = 8.0e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def workload():
    """(K, 64 depth frames, 64 extrinsics, 64 RGB images)."""
    K, depths, ext = ex.scene_frames(W, H, POSES)
    rng = np.random.default_rng(5)
    rgb = [rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(POSES)]
    rep = FRAMES // POSES
    return K, depths * rep, ext * rep, rgb * rep


def make(R, colour):
    length, R, trunc, origin = ex.volume_settings(R)
    return tp.UniformTSDFVolume(length, R, trunc, tp.TSDFVolumeColorType.RGB8 if colour else tp.TSDFVolumeColorType.NoColor, origin)


def one_call(vol, K, d, e, c):
    vol.integrate_batch(d, K, e, c, 1000.0, 6.0)


def many_calls(vol, K, d, e, c):
    for k in range(len(d)):
        vol.integrate(d[k], K, e[k], None if c is None else c[k], 1000.0, 6.0)


def touched_per_pass(R, colour, K, d, e, c):
    """Per pass of CHUNK frames the voxels it touches: each chunk goes into an emptied volume, the weights come back."""
    out = []
    with make(R, colour) as vol:
        for k in range(0, FRAMES, CHUNK):
            vol.reset()
            one_call(vol, K, d[k:k + CHUNK], e[k:k + CHUNK], None if c is None else c[k:k + CHUNK])
            out.append(int(np.count_nonzero(vol.extract_volume_tsdf()[:, 1])))
    return out


def run_setting(R, colour, K, d, e, c, reps, warmup, compare_colour):
    cc = c if colour else None
    res = dict(R=R, colour=bool(colour), voxel_bytes=32 if colour else 8)
    with make(R, colour) as a, make(R, colour) as b:
        one_call(a, K, d, e, cc)
        many_calls(b, K, d, e, cc)
        ta, tb = a.extract_volume_tsdf(), b.extract_volume_tsdf()
        res["same_bits_tsdf_weight"] = bool(np.array_equal(ta.view(np.uint32), tb.view(np.uint32)))
        res["observed_voxels"] = int(np.count_nonzero(ta[:, 1]))
        del ta, tb
        if colour and compare_colour:
            res["same_bits_colour"] = bool(a.extract_volume_color().tobytes() == b.extract_volume_color().tobytes())
        pc = a.extract_point_cloud()
        res["surface_points"] = len(pc.points)
        res["max_distance_to_surface"] = float(ex.distance_to_surface(pc.points).max())
        res["extract_point_cloud"] = timed(lambda: a.extract_point_cloud(), reps, warmup)
        res["extract_point_cloud_no_normals"] = timed(lambda: a.extract_point_cloud(normals=False), reps, warmup)
        res["voxel_points"] = len(a.extract_voxel_point_cloud().points)
        res["extract_voxel_point_cloud"] = timed(lambda: a.extract_voxel_point_cloud(), reps, warmup)
        res["integrate_one_call_64_frames"] = timed(lambda: one_call(a, K, d, e, cc), reps, warmup)
        res["integrate_64_calls"] = timed(lambda: many_calls(b, K, d, e, cc), reps, warmup)
    for key in ("integrate_one_call_64_frames", "integrate_64_calls"):
        res[key]["ms_per_frame"] = res[key]["median_ms"] / FRAMES
    return res


def restatement():
    import tsdf_reference as T
    K, d, e = ex.scene_frames(160, 120, 8)
    length, R, trunc, origin = ex.volume_settings(32)
    t = time.perf_counter()
    vol = T.Volume(length, R, trunc, T.NONE, origin)
    for k in range(8):
        vol.integrate(d[k], (K.fx, K.fy, K.cx, K.cy), e[k], None, 1000.0, 6.0)
    t1 = time.perf_counter()
    P, _, _ = vol.extract_point_cloud()
    t2 = time.perf_counter()
    with tp.UniformTSDFVolume(length, R, trunc, 0, origin) as g:
        g.integrate_batch(d, K, e, None, 1000.0, 6.0)
        same = g.extract_volume_tsdf().tobytes() == vol.tsdf_weight().tobytes() and g.extract_point_cloud().points.tobytes() == P.tobytes()
    return dict(R=32, frames=8, width=160, height=120, integrate_ms=1e3 * (t1 - t), extract_ms=1e3 * (t2 - t1), points=len(P),
                device_equals_restatement=bool(same))


def run_mesh(R, K, d, e, c, reps, warmup):
    res = dict(R=R, colour=True)
    with make(R, 1) as vol:
        one_call(vol, K, d, e, c)
        mesh = vol.extract_triangle_mesh(vertex_normals=True)
        res["vertices"], res["triangles"] = len(mesh.vertices), len(mesh.triangles)
        res["output_bytes"] = int(mesh.vertices.nbytes * 3 + mesh.triangles.nbytes)
        res["max_distance_to_surface"] = float(ex.distance_to_surface(mesh.vertices).max())
        again = vol.extract_triangle_mesh(vertex_normals=True)
        res["same_bits_twice"] = bool(again.vertices.tobytes() == mesh.vertices.tobytes() and again.triangles.tobytes() == mesh.triangles.tobytes()
                                      and again.vertex_normals.tobytes() == mesh.vertex_normals.tobytes())
        del mesh, again
        res["extract_triangle_mesh"] = timed(lambda: vol.extract_triangle_mesh(), reps, warmup)
        res["extract_triangle_mesh_with_normals"] = timed(lambda: vol.extract_triangle_mesh(vertex_normals=True), reps, warmup)
        nv, nt = C.c_int64(0), C.c_int64(0)
        res["counts_only_call"] = timed(lambda: vol._call(tp.lib().teaser_hip_tsdf_extract_triangle_mesh, 0, None, None, None, 0, None,
                                                          C.byref(nv), C.byref(nt)), reps, warmup)
        res["surface_points"] = len(vol.extract_point_cloud().points)
        res["extract_point_cloud"] = timed(lambda: vol.extract_point_cloud(), reps, warmup)
        res["extract_point_cloud_no_normals"] = timed(lambda: vol.extract_point_cloud(normals=False), reps, warmup)
    return res


def mesh_restatement(K, d, e, c):
    """The Python loop on the host at R = 64 (8 frames), on the volume the device integrated."""
    import tsdf_mesh_reference as M
    import tsdf_reference as T
    length, R, trunc, origin = ex.volume_settings(64)
    with make(64, 1) as g:
        one_call(g, K, d[:CHUNK], e[:CHUNK], c[:CHUNK])
        vol = T.Volume(length, R, trunc, T.RGB8, origin)
        tw = g.extract_volume_tsdf().reshape(R, R, R, 2)
        vol.tsdf[:], vol.weight[:], vol.color[:] = tw[..., 0], tw[..., 1], g.extract_volume_color().reshape(R, R, R, 3)
        t = time.perf_counter()
        ref = M.extract_triangle_mesh(vol, normals=True)
        t1 = time.perf_counter()
        mesh = g.extract_triangle_mesh(vertex_normals=True)
        t2 = time.perf_counter()
    same = (mesh.vertices.tobytes() == ref.vertices.tobytes() and mesh.triangles.tobytes() == ref.triangles.tobytes()
            and mesh.vertex_colors.tobytes() == ref.colors.tobytes() and mesh.vertex_normals.tobytes() == ref.normals.tobytes())
    return dict(R=64, frames=CHUNK, restatement_ms=1e3 * (t1 - t), device_ms_one_untimed_call=1e3 * (t2 - t1), vertices=len(ref.vertices),
                triangles=len(ref.triangles), device_equals_restatement=bool(same))


def run_ray_cast(R, K, d, e, c, reps, warmup):
    res = dict(R=R, colour=True, width=W, height=H)
    views = e[:POSES]
    with make(R, 1) as vol:
        one_call(vol, K, d, e, c)
        kw = dict(depth_max=6.0, weight_threshold=3.0)
        full = vol.ray_cast(K, views[0], **kw)
        again = vol.ray_cast(K, views[0], **kw)
        res["hits"], res["filled_share"] = full.hits, full.hits / float(W * H)
        res["same_bits_twice"] = bool(all(getattr(full, n).tobytes() == getattr(again, n).tobytes() for n in ("depth", "vertex_map", "normal_map", "color")))
        pts = full.vertex_map[full.depth > 0].astype(np.float64)
        res["max_distance_to_surface"] = float(ex.distance_to_surface(pts).max())
        res["output_bytes_all_maps"] = int(full.depth.nbytes + full.vertex_map.nbytes + full.normal_map.nbytes + full.color.nbytes)
        batch = vol.ray_cast_batch(K, views, **kw)
        res["batch_equals_single"] = bool(batch[0].depth.tobytes() == full.depth.tobytes() and batch[0].color.tobytes() == full.color.tobytes())
        res["ray_cast_all_maps"] = timed(lambda: vol.ray_cast(K, views[0], **kw), reps, warmup)
        res["ray_cast_depth_only"] = timed(lambda: vol.ray_cast(K, views[0], vertex_map=False, normal_map=False, color=False, **kw), reps, warmup)
        res["ray_cast_16_views_one_call"] = timed(lambda: vol.ray_cast_batch(K, views, **kw), reps, warmup)
        res["ray_cast_16_calls"] = timed(lambda: [vol.ray_cast(K, v, **kw) for v in views], reps, warmup)
        res["ray_cast_16_views_one_call_depth_only"] = timed(
            lambda: vol.ray_cast_batch(K, views, vertex_map=False, normal_map=False, color=False, **kw), reps, warmup)
        # the route without the ray cast: the surface rows down, then up again into a depth image
        cloud = vol.extract_point_cloud(normals=False)
        res["surface_points"] = len(cloud.points)
        img = tp.project_to_depth_image(cloud.points, W, H, K, views[0], depth_scale=1.0, depth_max=6.0)
        res["projected_filled_share"] = float(np.count_nonzero(img)) / float(W * H)
        res["extract_point_cloud_no_normals"] = timed(lambda: vol.extract_point_cloud(normals=False), reps, warmup)
        res["project_to_depth_image"] = timed(lambda: tp.project_to_depth_image(cloud.points, W, H, K, views[0], depth_scale=1.0, depth_max=6.0), reps, warmup)
        res["extract_then_project"] = timed(lambda: tp.project_to_depth_image(vol.extract_point_cloud(normals=False).points, W, H, K, views[0],
                                                                              depth_scale=1.0, depth_max=6.0), reps, warmup)
    return res


def ray_cast_restatement(K, d, e, c):
    """The numpy restatement at R = 64 (8 frames, a 160 x 120 view) on the volume the device integrated: equality and
    the steps per ray."""
    import tsdf_raycast_reference as RC
    import tsdf_reference as T
    length, R, trunc, origin = ex.volume_settings(64)
    Ks = tp.PinholeCameraIntrinsic(160, 120, K.fx / 4, K.fy / 4, (K.cx - 1.5) / 4, (K.cy - 1.5) / 4)
    with make(64, 1) as g:
        one_call(g, K, d[:CHUNK], e[:CHUNK], c[:CHUNK])
        vol = T.Volume(length, R, trunc, T.RGB8, origin)
        tw = g.extract_volume_tsdf().reshape(R, R, R, 2)
        vol.tsdf[:], vol.weight[:], vol.color[:] = tw[..., 0], tw[..., 1], g.extract_volume_color().reshape(R, R, R, 3)
        t = time.perf_counter()
        ref = RC.ray_cast(vol, (Ks.fx, Ks.fy, Ks.cx, Ks.cy), e[0], 160, 120, 0.1, 6.0, 3.0)
        t1 = time.perf_counter()
        got = g.ray_cast(Ks, e[0], depth_max=6.0, weight_threshold=3.0)
    same = (got.hits == ref.hits and got.depth.tobytes() == ref.depth.tobytes() and got.vertex_map.tobytes() == ref.vertex.tobytes()
            and got.normal_map.tobytes() == ref.normal.tobytes() and got.color.tobytes() == ref.color.tobytes())
    steps = ref.steps.ravel()
    return dict(R=64, frames=CHUNK, width=160, height=120, restatement_ms=1e3 * (t1 - t), hits=ref.hits, device_equals_restatement=bool(same),
                steps_max=int(steps.max()), steps_mean=float(steps.mean()), steps_median=float(np.median(steps)),
                steps_histogram_by_8=np.bincount(steps // 8).tolist())


def make_scalable(R, colour):
    length, R, trunc, _ = ex.volume_settings(R)
    return tp.ScalableTSDFVolume(length / R, trunc, tp.TSDFVolumeColorType.RGB8 if colour else tp.TSDFVolumeColorType.NoColor)


def run_scalable_ray_cast(R, K, d, e, c, reps, warmup):
    res = dict(R=R, colour=True, width=W, height=H)
    views = e[:POSES]
    kw = dict(depth_max=6.0, weight_threshold=3.0)
    only = dict(vertex_map=False, normal_map=False, color=False)
    with make_scalable(R, 1) as vol, make(R, 1) as dense:
        one_call(vol, K, d, e, c)
        one_call(dense, K, d, e, c)
        res["blocks"], res["scalable_bytes"], res["dense_bytes"] = vol.block_count, vol.block_count * vol.block_bytes, 32 * R ** 3
        full, again, ref = tp.ray_cast(vol, K, views[0], **kw), tp.ray_cast(vol, K, views[0], **kw), dense.ray_cast(K, views[0], **kw)
        res["hits"], res["filled_share"], res["dense_hits"] = full.hits, full.hits / float(W * H), ref.hits
        res["same_bits_twice"] = bool(all(getattr(full, n).tobytes() == getattr(again, n).tobytes() for n in ("depth", "vertex_map", "normal_map", "color")))
        both = (full.depth > 0) & (ref.depth > 0)
        res["pixels_hit_in_both"] = int(both.sum())
        res["max_depth_difference_to_dense_in_voxels"] = float(np.abs(full.depth[both] - ref.depth[both]).max() / vol.voxel_length)
        res["max_distance_to_surface"] = float(ex.distance_to_surface(full.vertex_map[full.depth > 0].astype(np.float64)).max())
        batch = vol.ray_cast_batch(K, views, **kw)
        res["batch_equals_single"] = bool(batch[0].depth.tobytes() == full.depth.tobytes() and batch[0].color.tobytes() == full.color.tobytes())
        # alternating: a scalable measurement, then the dense one of the same kind
        res["ray_cast_all_maps"] = timed(lambda: tp.ray_cast(vol, K, views[0], **kw), reps, warmup)
        res["dense_ray_cast_all_maps"] = timed(lambda: dense.ray_cast(K, views[0], **kw), reps, warmup)
        res["ray_cast_depth_only"] = timed(lambda: tp.ray_cast(vol, K, views[0], **only, **kw), reps, warmup)
        res["dense_ray_cast_depth_only"] = timed(lambda: dense.ray_cast(K, views[0], **only, **kw), reps, warmup)
        res["ray_cast_16_views_one_call"] = timed(lambda: vol.ray_cast_batch(K, views, **kw), reps, warmup)
        res["dense_ray_cast_16_views_one_call"] = timed(lambda: dense.ray_cast_batch(K, views, **kw), reps, warmup)
        res["ray_cast_16_views_one_call_depth_only"] = timed(lambda: vol.ray_cast_batch(K, views, **only, **kw), reps, warmup)
        cloud = vol.extract_point_cloud(normals=False)
        res["surface_points"] = len(cloud.points)
        img = tp.project_to_depth_image(cloud.points, W, H, K, views[0], depth_scale=1.0, depth_max=6.0)
        res["projected_filled_share"] = float(np.count_nonzero(img)) / float(W * H)
        res["extract_then_project"] = timed(lambda: tp.project_to_depth_image(vol.extract_point_cloud(normals=False).points, W, H, K, views[0],
                                                                              depth_scale=1.0, depth_max=6.0), reps, warmup)
    return res


def scalable_ray_cast_restatement(R, K, d, e):
    """The numpy restatement on the volume that was timed -- all 64 frames at the voxels of R, fused on the device; the
    tsdf and the weights do not depend on the colour, so a volume without colour is downloaded -- for a 160 x 120 view at
    the first pose: equality of the depth, vertex and normal maps and the hit count with the device's, and from the trace
    the steps, the steps in blocks that are not open and the block changes (directory searches) of every ray."""
    import stsdf_raycast_reference as SR
    import stsdf_reference as S
    import tsdf_reference as T
    length, R, trunc, _ = ex.volume_settings(R)
    Ks = tp.PinholeCameraIntrinsic(160, 120, K.fx / 4, K.fy / 4, (K.cx - 1.5) / 4, (K.cy - 1.5) / 4)
    with make_scalable(R, 0) as g:
        one_call(g, K, d, e, None)
        keys, tw, _ = g.extract_blocks()
        U = S.U
        # Open3D's voxel order (x U + y) U + z is the restatement's [x, y, z]
        vol = SR.volume_of_blocks(length / R, trunc, T.NONE, {tuple(int(v) for v in k): (tw[n, :, 0].reshape(U, U, U), tw[n, :, 1].reshape(U, U, U), None)
                                                             for n, k in enumerate(keys)})
        lat = SR.Lattice(vol)
        print("restatement: %d blocks packed, marching" % len(keys), file=sys.stderr, flush=True)
        trace = []
        t = time.perf_counter()
        ref = SR.ray_cast(vol, (Ks.fx, Ks.fy, Ks.cx, Ks.cy), e[0], 160, 120, 0.1, 6.0, 3.0, trace=trace, lat=lat)
        t1 = time.perf_counter()
        got = tp.ray_cast(g, Ks, e[0], depth_max=6.0, weight_threshold=3.0)
    same = (got.hits == ref.hits and got.depth.tobytes() == ref.depth.tobytes() and got.vertex_map.tobytes() == ref.vertex.tobytes()
            and got.normal_map.tobytes() == ref.normal.tobytes())
    n = 160 * 120
    steps, absent, changes, absent_changes = (np.zeros(n, dtype=np.int64) for _ in range(4))
    last = np.full((n, 3), np.nan, dtype=np.float32)
    for s in trace:
        steps += s.active
        absent += s.active & ~s.open
        moved = s.active & (s.B != last).any(axis=1)
        changes += moved
        absent_changes += moved & ~s.open
        last[s.active] = s.B[s.active]
    del trace
    assert (steps == ref.steps.ravel()).all()
    print("restatement: %.1f s, marching again without the skip" % (t1 - t), file=sys.stderr, flush=True)
    slow = SR.ray_cast(vol, (Ks.fx, Ks.fy, Ks.cx, Ks.cy), e[0], 160, 120, 0.1, 6.0, 3.0, skip=False, lat=lat)
    return dict(R=R, frames=len(d), width=160, height=120, blocks=len(keys), restatement_ms=1e3 * (t1 - t), hits=ref.hits,
                device_equals_restatement=bool(same), steps_max=int(steps.max()), steps_mean=float(steps.mean()),
                steps_median=float(np.median(steps)), steps_histogram_by_8=np.bincount(steps // 8).tolist(),
                steps_in_absent_blocks_mean=float(absent.mean()), share_of_steps_in_absent_blocks=float(absent.sum()) / float(steps.sum()),
                directory_searches_mean=float(changes.mean()), directory_searches_median=float(np.median(changes)),
                directory_searches_max=int(changes.max()), directory_searches_that_find_no_block_mean=float(absent_changes.mean()),
                steps_mean_without_skip=float(slow.steps.mean()), steps_max_without_skip=int(slow.steps.max()), hits_without_skip=slow.hits)


def run_scalable_mesh(R, K, d, e, c, reps, warmup):
    res = dict(R=R, colour=True)
    with make_scalable(R, 1) as vol, make(R, 1) as dense:
        one_call(vol, K, d, e, c)
        one_call(dense, K, d, e, c)
        res["blocks"], res["scalable_bytes"], res["dense_bytes"] = vol.block_count, vol.block_count * vol.block_bytes, 32 * R ** 3
        res["voxels_of_open_blocks"], res["dense_voxels"] = vol.block_count * 4096, R ** 3
        mesh = vol.extract_mesh(vertex_normals=True)
        res["vertices"], res["triangles"] = len(mesh.vertices), len(mesh.triangles)
        res["output_bytes"] = int(mesh.vertices.nbytes * 3 + mesh.triangles.nbytes)
        res["max_distance_to_surface"] = float(ex.distance_to_surface(mesh.vertices).max())
        again = vol.extract_mesh(vertex_normals=True)
        res["same_bits_twice"] = bool(again.vertices.tobytes() == mesh.vertices.tobytes() and again.triangles.tobytes() == mesh.triangles.tobytes()
                                      and again.vertex_normals.tobytes() == mesh.vertex_normals.tobytes())
        ref = dense.extract_triangle_mesh()
        res["dense_vertices"], res["dense_triangles"] = len(ref.vertices), len(ref.triangles)
        del mesh, again, ref
        nv, nt = C.c_int64(0), C.c_int64(0)
        # alternating: a scalable measurement, then the dense one of the same kind
        res["extract_mesh"] = timed(lambda: vol.extract_mesh(), reps, warmup)
        res["dense_extract_triangle_mesh"] = timed(lambda: dense.extract_triangle_mesh(), reps, warmup)
        res["extract_mesh_with_normals"] = timed(lambda: vol.extract_mesh(vertex_normals=True), reps, warmup)
        res["dense_extract_triangle_mesh_with_normals"] = timed(lambda: dense.extract_triangle_mesh(vertex_normals=True), reps, warmup)
        res["counts_only_call"] = timed(lambda: vol._call(tp.lib().teaser_hip_stsdf_extract_triangle_mesh, 0, None, None, None, 0, None,
                                                          C.byref(nv), C.byref(nt)), reps, warmup)
        res["dense_counts_only_call"] = timed(lambda: dense._call(tp.lib().teaser_hip_tsdf_extract_triangle_mesh, 0, None, None, None, 0, None,
                                                                  C.byref(nv), C.byref(nt)), reps, warmup)
        res["surface_points"] = len(vol.extract_point_cloud().points)
        res["extract_point_cloud"] = timed(lambda: vol.extract_point_cloud(), reps, warmup)
        res["extract_point_cloud_no_normals"] = timed(lambda: vol.extract_point_cloud(normals=False), reps, warmup)
    return res


def scalable_mesh_restatement(K, d, e, c):
    """The Python loop on the host at the voxels of R = 64 (8 frames), on the blocks the device integrated."""
    import stsdf_mesh_reference as SM
    import stsdf_raycast_reference as SR
    import stsdf_reference as S
    import tsdf_reference as T
    length, R, trunc, _ = ex.volume_settings(64)
    U = S.U
    with make_scalable(64, 1) as g:
        one_call(g, K, d[:CHUNK], e[:CHUNK], c[:CHUNK])
        keys, tw, col = g.extract_blocks()
        # Open3D's voxel order (x U + y) U + z is the restatement's [x, y, z]
        vol = SR.volume_of_blocks(length / R, trunc, T.RGB8, {tuple(int(v) for v in k): (tw[n, :, 0].reshape(U, U, U), tw[n, :, 1].reshape(U, U, U),
                                                                                       col[n].reshape(U, U, U, 3)) for n, k in enumerate(keys)})
        t = time.perf_counter()
        ref = SM.extract_triangle_mesh(vol, normals=True)
        t1 = time.perf_counter()
        mesh = g.extract_mesh(vertex_normals=True)
        t2 = time.perf_counter()
    blocks, cubes, crossing, differ = SM.face_statistics(vol)
    same = (mesh.vertices.tobytes() == ref.vertices.tobytes() and mesh.triangles.tobytes() == ref.triangles.tobytes()
            and mesh.vertex_colors.tobytes() == ref.colors.tobytes() and mesh.vertex_normals.tobytes() == ref.normals.tobytes())
    return dict(R=64, frames=CHUNK, blocks=blocks, active_cubes=cubes, active_cubes_with_a_local_index_of_15=crossing,
                edges_whose_creator_is_not_the_dense_one=differ, restatement_ms=1e3 * (t1 - t), device_ms_one_untimed_call=1e3 * (t2 - t1),
                vertices=len(ref.vertices), triangles=len(ref.triangles), device_equals_restatement=bool(same))


def run_scalable(R, colour, K, d, e, c, reps, warmup):
    cc = c if colour else None
    length, R, trunc, _ = ex.volume_settings(R)
    ctype = tp.TSDFVolumeColorType.RGB8 if colour else tp.TSDFVolumeColorType.NoColor
    res = dict(R=R, colour=bool(colour), voxel_length=length / R, sdf_trunc=trunc, dense_bytes=(32 if colour else 8) * R ** 3)
    phases = {}

    def fresh_one_call(vol):
        vol.reset()
        one_call(vol, K, d, e, cc)
        phases.setdefault("fresh", []).append(vol.last_phases_ms())

    def warm_one_call(vol):
        one_call(vol, K, d, e, cc)
        phases.setdefault("warm", []).append(vol.last_phases_ms())

    def fresh_many_calls(vol):
        vol.reset()
        many_calls(vol, K, d, e, cc)

    with tp.ScalableTSDFVolume(length / R, trunc, ctype) as a, tp.ScalableTSDFVolume(length / R, trunc, ctype) as b, make(R, colour) as dense:
        one_call(a, K, d, e, cc)
        many_calls(b, K, d, e, cc)
        res["touched_pairs"], res["blocks"], res["out_of_range"] = a.last_counts[0], a.block_count, a.last_counts[2]
        res["scalable_bytes"] = a.block_count * a.block_bytes
        ka, ta, ca = a.extract_blocks()
        kb, tb, cb = b.extract_blocks()
        res["same_bits_one_call_and_64_calls"] = bool(ka.tobytes() == kb.tobytes() and ta.tobytes() == tb.tobytes() and
                                                      (ca is None or ca.tobytes() == cb.tobytes()))
        del ta, tb, ca, cb
        pc = a.extract_point_cloud()
        res["surface_points"] = len(pc.points)
        res["max_distance_to_surface"] = float(ex.distance_to_surface(pc.points).max())
        res["voxel_points"] = len(a.extract_voxel_point_cloud().points)
        # alternating: a scalable measurement, then the dense one of the same kind
        res["extract_point_cloud"] = timed(lambda: a.extract_point_cloud(), reps, warmup)
        one_call(dense, K, d, e, cc)
        res["dense_extract_point_cloud"] = timed(lambda: dense.extract_point_cloud(), reps, warmup)
        res["dense_surface_points"] = len(dense.extract_point_cloud().points)
        res["extract_point_cloud_no_normals"] = timed(lambda: a.extract_point_cloud(normals=False), reps, warmup)
        res["extract_voxel_point_cloud"] = timed(lambda: a.extract_voxel_point_cloud(), reps, warmup)
        res["dense_extract_voxel_point_cloud"] = timed(lambda: dense.extract_voxel_point_cloud(), reps, warmup)
        res["integrate_one_call_64_frames_fresh"] = timed(lambda: fresh_one_call(a), reps, warmup)
        res["dense_integrate_one_call_64_frames"] = timed(lambda: one_call(dense, K, d, e, cc), reps, warmup)
        res["integrate_one_call_64_frames_warm"] = timed(lambda: warm_one_call(a), reps, warmup)
        res["integrate_64_calls_fresh"] = timed(lambda: fresh_many_calls(b), reps, warmup)
        res["dense_integrate_64_calls"] = timed(lambda: many_calls(dense, K, d, e, cc), reps, warmup)
        res["integrate_64_calls_warm"] = timed(lambda: many_calls(b, K, d, e, cc), reps, warmup)
    for key in list(res):
        if "integrate_" in key:
            res[key]["ms_per_frame"] = res[key]["median_ms"] / FRAMES
    for kind, rows in phases.items():
        med = np.median(np.array(rows[warmup:]), axis=0)
        res["phases_one_call_%s_ms" % kind] = dict(touch_and_readback=float(med[0]), directory_on_host=float(med[1]),
                                                   zeroing_and_integration=float(med[2]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--profile-workload", choices=["one_call", "calls", "extract", "mesh", "ray_cast", "scalable_ray_cast", "scalable_mesh"], default=None)
    ap.add_argument("--profile-R", type=int, default=512)
    ap.add_argument("--profile-colour", type=int, default=1)
    ap.add_argument("--mesh", action="store_true", help="measure the triangle mesh instead (profiles/tsdf_mesh/)")
    ap.add_argument("--ray-cast", action="store_true", help="measure the ray cast instead (profiles/tsdf_raycast/)")
    ap.add_argument("--scalable", action="store_true", help="measure the scalable volume instead (profiles/tsdf_scalable/)")
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_tsdf.py needs an MI355X: no HIP device visible")
    K, d, e, c = workload()
    if a.profile_workload == "scalable_ray_cast":
        with make_scalable(a.profile_R, 1) as vol, make(a.profile_R, 1) as dense:
            one_call(vol, K, d, e, c)
            one_call(dense, K, d, e, c)
            for rep in range(3):
                for v in (vol, dense):
                    tp.ray_cast(v, K, e[0], depth_max=6.0, weight_threshold=3.0)
                    v.ray_cast_batch(K, e[:POSES], depth_max=6.0, weight_threshold=3.0)
        return
    if a.profile_workload == "scalable_mesh":
        with make_scalable(a.profile_R, 1) as vol, make(a.profile_R, 1) as dense:
            one_call(vol, K, d, e, c)
            one_call(dense, K, d, e, c)
            for rep in range(3):
                vol.extract_mesh(vertex_normals=True)
                dense.extract_triangle_mesh(vertex_normals=True)
        return
    if a.profile_workload:
        cc = c if a.profile_colour else None
        with make(a.profile_R, a.profile_colour) as vol:
            for rep in range(3):
                if a.profile_workload == "one_call":
                    one_call(vol, K, d, e, cc)
                elif a.profile_workload == "calls":
                    many_calls(vol, K, d, e, cc)
                elif a.profile_workload == "mesh":
                    one_call(vol, K, d[:CHUNK], e[:CHUNK], None if cc is None else cc[:CHUNK])
                    vol.extract_triangle_mesh(vertex_normals=True)
                elif a.profile_workload == "ray_cast":
                    if rep == 0:
                        one_call(vol, K, d, e, cc)
                    vol.ray_cast(K, e[0], depth_max=6.0, weight_threshold=3.0)
                    vol.ray_cast_batch(K, e[:POSES], depth_max=6.0, weight_threshold=3.0)
                else:
                    one_call(vol, K, d[:CHUNK], e[:CHUNK], None if cc is None else cc[:CHUNK])
                    vol.extract_point_cloud()
                    vol.extract_voxel_point_cloud()
        return
    out = dict(workload=dict(width=W, height=H, frames=FRAMES, poses=POSES, chunk=CHUNK, hbm_peak=HBM_PEAK), settings=[])
    if a.scalable and a.ray_cast:
        for R in a.sizes:
            r = run_scalable_ray_cast(R, K, d, e, c, a.reps, a.warmup)
            print(json.dumps(r), flush=True)
            out["settings"].append(r)
        out["restatement"] = scalable_ray_cast_restatement(a.sizes[0], K, d, e)
        print(json.dumps(out["restatement"]), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    if a.scalable and a.mesh:
        for R in a.sizes:
            r = run_scalable_mesh(R, K, d, e, c, a.reps, a.warmup)
            print(json.dumps(r), flush=True)
            out["settings"].append(r)
        out["restatement"] = scalable_mesh_restatement(K, d, e, c)
        print(json.dumps(out["restatement"]), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    if a.scalable:
        for R in a.sizes:
            for colour in (0, 1):
                r = run_scalable(R, colour, K, d, e, c, a.reps, a.warmup)
                print(json.dumps(r), flush=True)
                out["settings"].append(r)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    if a.ray_cast:
        for R in a.sizes:
            r = run_ray_cast(R, K, d, e, c, a.reps, a.warmup)
            print(json.dumps(r), flush=True)
            out["settings"].append(r)
        out["restatement"] = ray_cast_restatement(K, d, e, c)
        print(json.dumps(out["restatement"]), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    if a.mesh:
        for R in a.sizes:
            r = run_mesh(R, K, d, e, c, a.reps, a.warmup)
            print(json.dumps(r), flush=True)
            out["settings"].append(r)
        out["restatement"] = mesh_restatement(K, d, e, c)
        print(json.dumps(out["restatement"]), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    for R in a.sizes:
        for colour in (0, 1):
            r = run_setting(R, colour, K, d, e, c, a.reps, a.warmup, compare_colour=R <= 256)
            if R <= 256:
                r["touched_voxels_per_pass"] = touched_per_pass(R, colour, K, d, e, c)
            print(json.dumps(r), flush=True)
            out["settings"].append(r)
    out["restatement"] = restatement()
    print(json.dumps(out["restatement"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
