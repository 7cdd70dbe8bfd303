#!/usr/bin/env python3
"""Dense SLAM on depth alone: integrate -> ray cast -> track -> integrate, the loop of KinectFusion and of Open3D's
t.pipelines.slam.Model, with the model in a TSDF volume on the MI355X.

The scene and the camera path are those of examples/teaser_python_odometry.py: the analytic wall with its balls and a
camera that moves three centimetres and about a degree per frame; the poses are known.  Then:

    frame 0 integrated at its TRUE pose                        (UniformTSDFVolume.integrate; a volume without colour)
    every later frame k:
      tracked against the model from the pose of frame k - 1   (track_frame_to_model: the model's depth ray cast at that
                                                                pose, depth odometry of the frame against it, the pose
                                                                camera_to_world_init @ T)
      integrated at the TRACKED pose

It prints, per frame, the drift of the tracked pose against the true one (rotation in degrees, translation in metres)
beside the drift of not tracking at all (holding the pose of the frame before).  With --scalable the model is a
ScalableTSDFVolume with the same voxels and truncation.  Exit code 77: no MI355X visible.  Usage:

    python examples/teaser_python_slam.py [--width 320 --height 240] [--frames 8] [--resolution 128] [--scalable]
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
odo = importlib.import_module("teaser_python_odometry")     # the camera path and the renderer

DEPTH_MAX = 6.0


def tracking_option():
    """Open3D's defaults with the scene's depth range."""
    return tp.DepthOdometryOption(depth_max=DEPTH_MAX)


def make_volume(resolution, scalable):
    length, R, trunc, origin = fusion.volume_settings(resolution)
    if scalable:
        return tp.ScalableTSDFVolume(length / R, trunc, tp.TSDFVolumeColorType.NoColor)
    return tp.UniformTSDFVolume(length, R, trunc, tp.TSDFVolumeColorType.NoColor, origin)


def drift(estimate, truth):
    """(rotation in degrees, translation in metres) between two camera-to-world poses."""
    E = np.linalg.inv(truth) @ estimate
    return float(np.degrees(np.arccos(min(1.0, max(-1.0, (np.trace(E[:3, :3]) - 1.0) / 2.0))))), float(np.linalg.norm(E[:3, 3]))


def track_sequence(K, depths, first_pose, resolution, scalable, option=None):
    """The loop: (the tracked camera-to-world poses, one TrackingResult per frame from the second on)."""
    option = tracking_option() if option is None else option
    poses, tracked = [np.array(first_pose, dtype=np.float64)], []
    with make_volume(resolution, scalable) as vol:
        vol.integrate(depths[0], K, np.linalg.inv(poses[0]), depth_scale=1000.0, depth_trunc=DEPTH_MAX)
        for depth in depths[1:]:
            tr = tp.track_frame_to_model(vol, depth, K, poses[-1], option, weight_threshold=1.0)
            if not tr.success:
                raise RuntimeError("tracking failed at frame %d" % len(poses))
            tracked.append(tr)
            poses.append(tr.camera_to_world)
            vol.integrate(depth, K, np.linalg.inv(poses[-1]), depth_scale=1000.0, depth_trunc=DEPTH_MAX)
    return poses, tracked


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--scalable", action="store_true", help="keep the model in a ScalableTSDFVolume with the same voxels")
    a = ap.parse_args(argv)
    if a.frames < 2:
        sys.exit("--frames must be at least 2")
    if tp.device_count() < 1:
        print("this example needs an MI355X: no HIP device visible", file=sys.stderr)
        sys.exit(77)
    K, truth, depths, _ = odo.sequence(a.width, a.height, a.frames)
    t0 = time.perf_counter()
    poses, tracked = track_sequence(K, depths, truth[0], a.resolution, a.scalable)
    t1 = time.perf_counter()
    print("%d frames of %d x %d tracked against a %s model of %d^3 voxels' size, %.1f ms per frame" %
          (a.frames - 1, a.width, a.height, "scalable" if a.scalable else "dense", a.resolution, 1e3 * (t1 - t0) / (a.frames - 1)))
    for k in range(1, a.frames):
        r = tracked[k - 1].result
        dr, dt = drift(poses[k], truth[k])
        hr, ht = drift(poses[k - 1], truth[k])
        print("frame %d: drift %.6f deg %.6f m (untracked %.6f deg %.6f m), %d iterations, fitness %.4f, rmse %.6f m" %
              (k, dr, dt, hr, ht, r.iterations, r.fitness, r.inlier_rmse))


if __name__ == "__main__":
    main()
