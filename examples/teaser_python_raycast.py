#!/usr/bin/env python3
"""Frame-to-model tracking, the KinectFusion loop, with the model never leaving the MI355X.

The scene and the camera path are those of examples/teaser_python_odometry.py: the analytic wall with its balls, painted
with an intensity that is a function of the surface point, and a camera that moves a few centimetres per frame.  Then:

    all frames but the last integrated with their poses   (UniformTSDFVolume.integrate_batch, a Gray32 volume)
 -> the model rendered at the second-to-last pose         (UniformTSDFVolume.ray_cast: depth, normals and intensity)
 -> odometry of that MODEL frame against the last frame   (compute_rgbd_odometry: the ray cast's float32 metres and
                                                           float32 intensity go in as they are)

It prints how far the model's depth lies from the analytically rendered depth of the same pose, and the pose error of
frame-to-model odometry beside that of frame-to-frame odometry (the second-to-last camera frame against the last).
With --scalable the model is a ScalableTSDFVolume with the same voxels and truncation -- only the blocks of 16^3 voxels
near the surface exist, and the space needs no bounds -- rendered by tp.ray_cast, which serves either volume class.
Exit code 77: no MI355X visible.  Usage:

    python examples/teaser_python_raycast.py [--width 320 --height 240] [--frames 8] [--resolution 128] [--scalable]
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
odo = importlib.import_module("teaser_python_odometry")     # the camera path, the paint and the pose error

DEPTH_MAX = 6.0


def metres(depth):
    """A 16-bit millimetre frame as the float32 metres a model frame has."""
    return depth.astype(np.float32) / np.float32(1000.0)


def depth_error(model, analytic, voxel):
    """|model - analytic| in voxels over the pixels both see: (pixels, median, 95th percentile, maximum)."""
    both = (model > 0) & (analytic > 0)
    e = np.abs(model[both].astype(np.float64) - analytic[both].astype(np.float64)) / voxel
    return int(both.sum()), float(np.median(e)), float(np.percentile(e, 95.0)), float(e.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--scalable", action="store_true", help="keep the model in a ScalableTSDFVolume with the same voxels")
    a = ap.parse_args()
    if a.frames < 3:
        sys.exit("--frames must be at least 3")
    if tp.device_count() < 1:
        print("this example needs an MI355X: no HIP device visible", file=sys.stderr)
        sys.exit(77)
    K, poses, depths, paints = odo.sequence(a.width, a.height, a.frames)
    length, R, trunc, origin = fusion.volume_settings(a.resolution)
    if a.scalable:
        vol = tp.ScalableTSDFVolume(length / R, trunc, tp.TSDFVolumeColorType.Gray32)
    else:
        vol = tp.UniformTSDFVolume(length, R, trunc, tp.TSDFVolumeColorType.Gray32, origin)
    with vol:
        t0 = time.perf_counter()
        vol.integrate_batch(depths[:-1], K, [np.linalg.inv(p) for p in poses[:-1]], paints[:-1], depth_scale=1000.0, depth_trunc=DEPTH_MAX)
        t1 = time.perf_counter()
        model = tp.ray_cast(vol, K, np.linalg.inv(poses[-2]), depth_max=DEPTH_MAX, weight_threshold=min(3.0, a.frames - 1.0))
        t2 = time.perf_counter()
        voxel = vol.voxel_length
        blocks = vol.block_count if a.scalable else 0
    if a.scalable:
        print("integration: %d frames of %d x %d into %d blocks of 16^3 voxels, %.1f ms" % (a.frames - 1, a.width, a.height, blocks, 1e3 * (t1 - t0)))
    else:
        print("integration: %d frames of %d x %d into %d^3 voxels, %.1f ms" % (a.frames - 1, a.width, a.height, R, 1e3 * (t1 - t0)))
    print("ray cast at pose %d: %d of %d pixels hit, %.1f ms" % (a.frames - 2, model.hits, a.width * a.height, 1e3 * (t2 - t1)))
    n, med, p95, worst = depth_error(model.depth, metres(depths[-2]), voxel)
    print("model depth against the analytic depth: %d pixels, median %.17g, 95th percentile %.17g, max %.6f voxels" % (n, med, p95, worst))
    last = tp.RGBDImage(paints[-1], metres(depths[-1]), depth_scale=1.0)
    camera = tp.RGBDImage(paints[-2], metres(depths[-2]), depth_scale=1.0)
    option = tp.OdometryOption(depth_max=DEPTH_MAX)
    truth = odo.true_motion(poses, a.frames - 2)
    ok = True
    for name, source in (("frame-to-model", model.as_rgbd_image()), ("frame-to-frame", camera)):
        success, T, _ = tp.compute_rgbd_odometry(source, last, K, None, tp.RGBDOdometryJacobianFromHybridTerm, option)
        er, et = odo.pose_error(T, truth)
        print("%s odometry: success %d, rotation error %.17g deg, translation error %.17g m" % (name, success, er, et))
        ok = ok and success
    r0, t0_ = odo.pose_error(np.eye(4), truth)
    print("identity guess: rotation error %.6f deg, translation error %.6f m" % (r0, t0_))
    if not ok:
        sys.exit("odometry failed")


if __name__ == "__main__":
    main()
