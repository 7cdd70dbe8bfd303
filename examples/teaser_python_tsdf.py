#!/usr/bin/env python3
"""From depth frames and their camera poses to one fused cloud, the volume never leaving the MI355X.

The scene is the analytic one of examples/teaser_python_rgbd.py: a tilted wall with twenty balls half sunk into it, so
that every pixel's depth is a closed-form ray hit.  A handful of 16-bit depth frames are rendered from known camera
poses (the poses a multiway registration such as examples/teaser_python_multiway.py ends with), then:

    all frames integrated in ONE call   (UniformTSDFVolume.integrate_batch: two bytes per pixel go up)
 -> the surface extracted               (extract_point_cloud: points and normals come back)

It prints the number of extracted points and the largest distance from an extracted point to the analytic surface (the
nearer of the wall and the balls' spheres).  With --mesh PATH the triangle mesh is extracted too (extract_triangle_mesh:
marching cubes on the device) and written to PATH as a PLY file.  With --scalable the same frames also go into a
ScalableTSDFVolume with the same voxels, which needs no cube around the scene: it prints the blocks the frames opened and
the device bytes they hold beside the dense cube's, and the same two figures for its cloud; with --mesh PATH its mesh is
extracted as well (the same line, and PATH then holds the scalable volume's mesh, not the cube's).  Usage:

    python examples/teaser_python_tsdf.py [--width 320 --height 240] [--resolution 128] [--frames 8] [--mesh PATH] [--scalable]
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
scene = importlib.import_module("teaser_python_rgbd")  # the renderer and the scene: imported, not copied

LENGTH, ORIGIN = 3.0, (-1.5, -1.5, 1.2)    # the cube around the wall and its balls


def camera_poses(n):
    """n camera-to-world poses on a small arc in front of the wall."""
    poses = []
    for k in range(n):
        a = 2.0 * np.pi * k / max(n, 1)
        pose = np.eye(4)
        pose[:3, :3] = scene.rotation(np.radians(-3.0 + 2.0 * np.sin(a)), np.radians(6.0 * np.cos(a)))
        pose[:3, 3] = [0.25 * np.cos(a), 0.15 * np.sin(a), 0.02 * k]
        poses.append(pose)
    return poses


def scene_frames(width, height, n):
    """(intrinsic, depth frames, extrinsics): extrinsic = world to camera, the inverse of the pose."""
    K = tp.PinholeCameraIntrinsic(width, height, 0.95 * width, 0.95 * width, (width - 1) / 2.0, (height - 1) / 2.0)
    poses = camera_poses(n)
    return K, [scene.render_depth(K, p) for p in poses], [np.linalg.inv(p) for p in poses]


def distance_to_surface(points):
    """Per point the distance to the nearer of the wall's plane and the balls' spheres."""
    d = np.abs(points @ scene.PLANE_N - scene.PLANE_D)
    for c, r in scene.SPHERES:
        d = np.minimum(d, np.abs(np.linalg.norm(points - np.array(c), axis=1) - r))
    return d


def volume_settings(resolution):
    """(length, resolution, sdf_trunc, origin): the truncation is four voxels."""
    return LENGTH, resolution, 4.0 * LENGTH / resolution, ORIGIN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--mesh", default=None, help="also extract the triangle mesh and write it to this PLY file")
    ap.add_argument("--scalable", action="store_true", help="also fuse the frames in a ScalableTSDFVolume with the same voxels")
    a = ap.parse_args()
    K, depths, extrinsics = scene_frames(a.width, a.height, a.frames)
    length, R, trunc, origin = volume_settings(a.resolution)
    t0 = time.perf_counter()
    vol = tp.UniformTSDFVolume(length, R, trunc, tp.TSDFVolumeColorType.NoColor, origin)
    t1 = time.perf_counter()
    vol.integrate_batch(depths, K, extrinsics, depth_scale=1000.0, depth_trunc=6.0)
    t2 = time.perf_counter()
    cloud = vol.extract_point_cloud()
    t3 = time.perf_counter()
    print("volume: %d^3 voxels of %.4f, truncation %.4f (created in %.1f ms)" % (R, vol.voxel_length, trunc, 1e3 * (t1 - t0)))
    print("integration: %d frames of %d x %d in one call, %.1f ms" % (len(depths), a.width, a.height, 1e3 * (t2 - t1)))
    print("extraction: %d points with normals, %.1f ms" % (len(cloud.points), 1e3 * (t3 - t2)))
    d = distance_to_surface(cloud.points)
    print("distance to the analytic surface: max %.17g, mean %.6f (voxel %.6f)" % (d.max(), d.mean(), vol.voxel_length))
    if a.mesh:
        report_mesh(vol, a.mesh, "mesh")
    vol.close()
    if a.scalable:
        run_scalable(a, K, depths, extrinsics, length / R, trunc, 8 * R ** 3)


def report_mesh(vol, path, label):
    """The triangle mesh of either volume class (marching cubes on the device), written to `path` as a PLY file."""
    t0 = time.perf_counter()
    mesh = tp.extract_triangle_mesh(vol)
    t1 = time.perf_counter()
    tp.write_triangle_mesh(path, mesh)
    dm = distance_to_surface(mesh.vertices)
    print("%s: %d vertices, %d triangles, %.1f ms; distance to the analytic surface: max %.6f; written to %s"
          % (label, len(mesh.vertices), len(mesh.triangles), 1e3 * (t1 - t0), dm.max() if len(dm) else 0.0, path))


def run_scalable(a, K, depths, extrinsics, voxel_length, trunc, dense_bytes):
    """The same frames in blocks of 16^3 voxels: no cube, no origin."""
    t0 = time.perf_counter()
    with tp.ScalableTSDFVolume(voxel_length, trunc, tp.TSDFVolumeColorType.NoColor) as vol:
        vol.integrate_batch(depths, K, extrinsics, depth_scale=1000.0, depth_trunc=6.0)
        t1 = time.perf_counter()
        cloud = vol.extract_point_cloud()
        t2 = time.perf_counter()
        touched, opened, _ = vol.last_counts
        held = vol.block_count * vol.block_bytes
        print("scalable volume: voxels of %.4f in blocks of 16^3, truncation %.4f, every 4th pixel touches" % (voxel_length, trunc))
        print("scalable integration: %d frames in one call, %.1f ms; %d blocks opened (%d frame-block pairs), "
              "%d bytes held beside the dense cube's %d" % (len(depths), 1e3 * (t1 - t0), opened, touched, held, dense_bytes))
        print("scalable extraction: %d points with normals, %.1f ms" % (len(cloud.points), 1e3 * (t2 - t1)))
        d = distance_to_surface(cloud.points)
        print("scalable distance to the analytic surface: max %.17g, mean %.6f" % (d.max() if len(d) else 0.0, d.mean() if len(d) else 0.0))
        if a.mesh:
            report_mesh(vol, a.mesh, "scalable mesh")


if __name__ == "__main__":
    main()
