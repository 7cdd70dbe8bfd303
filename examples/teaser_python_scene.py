#!/usr/bin/env python3
"""A mesh as the TARGET of queries: the fused model of examples/teaser_python_raycast.py turned into a triangle mesh,
put into a RaycastingScene and looked at again.

    all frames but the last integrated with their poses   (UniformTSDFVolume.integrate_batch)
 -> the triangle mesh of the volume                       (UniformTSDFVolume.extract_triangle_mesh)
 -> a scene over that mesh                                (RaycastingScene.add_triangles: a BVH built on the device)
 -> the mesh rendered from the held-out last pose         (RaycastingScene.render_depth: float32 metres, 0 = nothing)
 -> the volume rendered from the same pose                (UniformTSDFVolume.ray_cast), and the difference of the two
 -> the distance from the volume's point cloud to the mesh (extract_point_cloud -> RaycastingScene.compute_distance)

Both renderings use rays through the pixels' corners (pixel_offset 0, the convention of the depth frames), so they differ
only in how each finds the zero crossing of the TSDF: the mesh interpolates along lattice edges, the ray cast along the
ray.  The points of extract_point_cloud lie on lattice edges by the rule the mesh vertices follow, so most of them ARE
mesh vertices up to the rounding of the vertices to float32.
Exit code 77: no MI355X visible.  Usage:

    python examples/teaser_python_scene.py [--width 320 --height 240] [--frames 8] [--resolution 128]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
tp = importlib.import_module("teaser-plusplus_amd")
fusion = importlib.import_module("teaser_python_tsdf")      # the volume's settings
odo = importlib.import_module("teaser_python_odometry")     # the scene and the camera path

DEPTH_MAX = 6.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=128)
    a = ap.parse_args()
    if a.frames < 3:
        sys.exit("--frames must be at least 3")
    if tp.device_count() < 1:
        print("this example needs an MI355X: no HIP device visible", file=sys.stderr)
        sys.exit(77)
    K, poses, depths, _ = odo.sequence(a.width, a.height, a.frames)
    length, R, trunc, origin = fusion.volume_settings(a.resolution)
    held_out = np.linalg.inv(poses[-1])
    with tp.UniformTSDFVolume(length, R, trunc, tp.TSDFVolumeColorType.NoColor, origin) as vol:
        vol.integrate_batch(depths[:-1], K, [np.linalg.inv(p) for p in poses[:-1]], depth_scale=1000.0, depth_trunc=DEPTH_MAX)
        mesh = vol.extract_triangle_mesh()
        cloud = vol.extract_point_cloud(normals=False)
        model = vol.ray_cast(K, held_out, depth_max=DEPTH_MAX, weight_threshold=1.0, vertex_map=False, normal_map=False)
        voxel = vol.voxel_length
    print("mesh: %d vertices, %d triangles from %d frames in %d^3 voxels" % (len(mesh.vertices), len(mesh.triangles), a.frames - 1, R))
    with tp.RaycastingScene() as scene:
        t0 = time.perf_counter()
        scene.add_triangles(mesh)
        scene.commit()
        t1 = time.perf_counter()
        depth = scene.render_depth(K, held_out, depth_max=DEPTH_MAX)
        t2 = time.perf_counter()
        dist = scene.compute_distance(cloud.points)
        t3 = time.perf_counter()
    print("scene: %d triangles built in %.1f ms; %d x %d view %.1f ms; %d closest-point queries %.1f ms"
          % (len(mesh.triangles), 1e3 * (t1 - t0), a.width, a.height, 1e3 * (t2 - t1), len(dist), 1e3 * (t3 - t2)))
    both = (depth > 0) & (model.depth > 0)
    e = np.abs(depth[both].astype(np.float64) - model.depth[both].astype(np.float64)) / voxel
    print("mesh render against the TSDF ray cast at the held-out pose: %d mesh pixels, %d ray-cast pixels, %d both, "
          "median %.17g, 95th percentile %.17g, max %.6f voxels"
          % (int((depth > 0).sum()), int((model.depth > 0).sum()), int(both.sum()), float(np.median(e)), float(np.percentile(e, 95.0)), float(e.max())))
    d = dist.astype(np.float64)
    print("scan to mesh: %d points, median %.17g m, 95th percentile %.17g m, max %.17g m (voxel %.6f m)"
          % (len(d), float(np.median(d)), float(np.percentile(d, 95.0)), float(d.max()), voxel))
    if both.sum() == 0 or not np.isfinite(d).all():
        sys.exit("the mesh and the volume do not see each other")


if __name__ == "__main__":
    main()
