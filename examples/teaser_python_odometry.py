#!/usr/bin/env python3
"""From a short RGB-D sequence to camera poses and one fused cloud: the first stage of a reconstruction pipeline on the
MI355X, with nothing but the frames given.

The scene is the analytic one of examples/teaser_python_rgbd.py (a tilted wall with twenty balls half sunk into it: every
pixel's depth is a closed-form ray hit), painted with an intensity that is a function of the surface point, so that two
views agree on it.  A camera moves a few centimetres and a fraction of a degree per frame.  Then:

    odometry on ALL consecutive pairs in ONE call   (compute_rgbd_odometry_batch)
 -> the poses chained from the first frame's
 -> a PoseGraph of the transformations and their information matrices (what a loop closure would be added to)
 -> the frames integrated with the ESTIMATED poses   (UniformTSDFVolume.integrate_batch)
 -> the surface extracted

It prints the pose errors against the truth and the fused cloud's distance to the analytic surface, beside the figure the
KNOWN poses give.  Exit code 77: no MI355X visible.  Usage:

    python examples/teaser_python_odometry.py [--width 320 --height 240] [--frames 8] [--resolution 128]
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
fusion = importlib.import_module("teaser_python_tsdf")  # the volume's settings and the distance to the surface


def trajectory(n):
    """n camera-to-world poses: three centimetres and about a degree from one frame to the next."""
    poses = []
    for k in range(n):
        pose = np.eye(4)
        pose[:3, :3] = scene.rotation(np.radians(-3.0 + 0.5 * k), np.radians(-2.0 + 0.9 * k))
        pose[:3, 3] = [-0.10 + 0.03 * k, 0.01 * k, 0.005 * k]
        poses.append(pose)
    return poses


def intensity(K, depth, pose):
    """float32, height x width: the paint of the surface point every pixel sees (0.5 where it sees nothing)."""
    i, j = np.meshgrid(np.arange(K.height, dtype=np.float64), np.arange(K.width, dtype=np.float64), indexing="ij")
    z = depth.astype(np.float64) / 1000.0
    P = np.stack([(j - K.cx) / K.fx * z, (i - K.cy) / K.fy * z, z], axis=2) @ pose[:3, :3].T + pose[:3, 3]
    paint = (0.5 + 0.2 * np.sin(9.0 * P[:, :, 0] + 2.0 * P[:, :, 2]) * np.cos(7.0 * P[:, :, 1])
             + 0.15 * np.sin(5.0 * P[:, :, 0] - 11.0 * P[:, :, 1]))
    return np.where(depth > 0, paint, 0.5).astype(np.float32)


def sequence(width, height, n):
    """(intrinsic, poses, depth frames, intensity frames)."""
    K = tp.PinholeCameraIntrinsic(width, height, 0.95 * width, 0.95 * width, (width - 1) / 2.0, (height - 1) / 2.0)
    poses = trajectory(n)
    depths = [scene.render_depth(K, p) for p in poses]
    return K, poses, depths, [intensity(K, d, p) for d, p in zip(depths, poses)]


def true_motion(poses, k):
    """Frame k to frame k + 1: what odometry estimates."""
    return np.linalg.inv(poses[k + 1]) @ poses[k]


def pose_error(estimate, truth):
    """(rotation in degrees, translation in metres) of estimate against truth."""
    E = estimate @ np.linalg.inv(truth)
    return np.degrees(np.arccos(min(1.0, max(-1.0, (np.trace(E[:3, :3]) - 1.0) / 2.0)))), float(np.linalg.norm(E[:3, 3]))


def chain(first, motions):
    """Camera-to-world poses from the first one and the frame-to-frame motions."""
    poses = [first]
    for T in motions:
        poses.append(poses[-1] @ np.linalg.inv(T))
    return poses


def fuse(K, depths, poses, resolution):
    length, R, trunc, origin = fusion.volume_settings(resolution)
    with tp.UniformTSDFVolume(length, R, trunc, tp.TSDFVolumeColorType.NoColor, origin) as vol:
        vol.integrate_batch(depths, K, [np.linalg.inv(p) for p in poses], depth_scale=1000.0, depth_trunc=6.0)
        return vol.extract_point_cloud(normals=False).points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=128)
    a = ap.parse_args()
    if tp.device_count() < 1:
        print("this example needs an MI355X: no HIP device visible", file=sys.stderr)
        sys.exit(77)
    K, poses, depths, paints = sequence(a.width, a.height, a.frames)
    frames = [tp.RGBDImage.create_from_color_and_depth(c, d, depth_scale=1000.0, depth_trunc=6.0) for c, d in zip(paints, depths)]
    option = tp.OdometryOption(depth_max=6.0)
    t0 = time.perf_counter()
    results = tp.compute_rgbd_odometry_batch(frames[:-1], frames[1:], K, None, tp.RGBDOdometryJacobianFromHybridTerm, option)
    t1 = time.perf_counter()
    print("odometry: %d pairs of %d x %d in one call, %.1f ms" % (len(results), a.width, a.height, 1e3 * (t1 - t0)))
    worst_r = worst_t = 0.0
    for k, r in enumerate(results):
        truth = true_motion(poses, k)
        r0, t0_ = pose_error(np.eye(4), truth)
        er, et = pose_error(r.transformation, truth)
        worst_r, worst_t = max(worst_r, er), max(worst_t, et)
        print("  pair %d -> %d: success %d, %d correspondences, rotation error %.4f deg (identity guess %.4f), translation error "
              "%.5f m (identity guess %.5f)" % (k, k + 1, r.success, r.count, er, r0, et, t0_))
    print("pair errors: max rotation %.17g deg, max translation %.17g m" % (worst_r, worst_t))
    estimated = chain(poses[0], [r.transformation for r in results])
    dr, dt = pose_error(estimated[-1], poses[-1])
    print("chained pose of the last frame: rotation error %.17g deg, translation error %.17g m" % (dr, dt))
    graph = tp.PoseGraph([tp.PoseGraphNode(p) for p in estimated],
                         [tp.PoseGraphEdge(k, k + 1, r.transformation, r.information, uncertain=False) for k, r in enumerate(results)])
    print("pose graph: %d nodes, %d odometry edges, smallest information diagonal %.1f" %
          (len(graph.nodes), len(graph.edges), min(float(np.diag(e.information).min()) for e in graph.edges)))
    cloud, known = fuse(K, depths, estimated, a.resolution), fuse(K, depths, poses, a.resolution)
    d, dk = fusion.distance_to_surface(cloud), fusion.distance_to_surface(known)
    print("fused cloud, estimated poses: %d points, distance to the analytic surface max %.17g, mean %.6f" % (len(cloud), d.max(), d.mean()))
    print("fused cloud, known poses:     %d points, distance to the analytic surface max %.17g, mean %.6f" % (len(known), dk.max(), dk.mean()))
    if not all(r.success for r in results):
        sys.exit("a pair failed")


if __name__ == "__main__":
    main()
