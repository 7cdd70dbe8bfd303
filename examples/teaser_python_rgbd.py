#!/usr/bin/env python3
"""From two depth frames to a registration and back to a picture, everything on the MI355X.

The scene is analytic: a tilted wall (a plane) with twenty balls (spheres) of different sizes half sunk into it, so that
every pixel's depth is a closed-form ray hit and the true pose between the two cameras is known.  (One ball in front of a
wall would not do: that scene is symmetric about the ball's axis and fixes no pose.)  Two 16-bit depth frames are
rendered from two camera poses (millimetres, like a depth camera's), then:

    unproject both frames in ONE call   (create_point_cloud_from_depth_image_batch, each in its own camera's frame)
 -> voxel down-sampling                 (voxel_down_sample_batch)
 -> FPFH, mutual nearest neighbours     (FPFHEstimation, Matcher)
 -> TEASER++                            (RobustRegistrationSolver)
 -> ICP seeded with the TEASER++ pose   (registration_icp)
 -> the registered source projected into the target's camera (project_to_depth_image with the estimated pose as the
    extrinsic), compared pixel by pixel with the target frame.

It prints the error of the recovered pose against the planted one and the share of target pixels whose projected depth
agrees with the frame within a voxel.  Usage:

    python examples/teaser_python_rgbd.py [--width 320 --height 240] [--voxel 0.05] [--icp-iterations 50]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
tp = importlib.import_module("teaser-plusplus_amd")

PLANE_N = np.array([0.1, -0.2, 1.0]) / np.linalg.norm([0.1, -0.2, 1.0])   # the wall: PLANE_N . X = PLANE_D
PLANE_D = 2.6


def bumps(seed=11):
    """Twenty balls half sunk into the wall on a jittered 5 x 4 grid, radii 0.10 .. 0.25: [(centre, radius)]."""
    rng = np.random.default_rng(seed)
    out = []
    for gy in range(4):
        for gx in range(5):
            x, y = -1.0 + 0.5 * gx + rng.uniform(-0.12, 0.12), -0.75 + 0.5 * gy + rng.uniform(-0.12, 0.12)
            z = (PLANE_D - PLANE_N[0] * x - PLANE_N[1] * y) / PLANE_N[2] - rng.uniform(0.0, 0.15)
            out.append(((x, y, z), rng.uniform(0.10, 0.25)))
    return out


SPHERES = bumps()


def rotation(rx, ry):
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    return np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


def render_depth(K, pose):
    """The depth frame (uint16, millimetres; 0 where a ray hits nothing) of the scene seen from `pose` (camera to
    world): per pixel the nearest of the closed-form ray hits.  The ray of pixel (i, j) is ((j - cx) / fx, (i - cy) / fy,
    1) in the camera's frame, so the ray parameter IS the depth."""
    i, j = np.meshgrid(np.arange(K.height, dtype=np.float64), np.arange(K.width, dtype=np.float64), indexing="ij")
    d = np.stack([(j - K.cx) / K.fx, (i - K.cy) / K.fy, np.ones_like(i)], axis=2) @ pose[:3, :3].T
    o = pose[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (PLANE_D - PLANE_N @ o) / (d @ PLANE_N)
        t = np.where(t > 0, t, np.inf)
        for c, r in SPHERES:
            oc = o - np.array(c)
            a, b, cc = (d * d).sum(axis=2), 2.0 * (d @ oc), oc @ oc - r * r
            disc = b * b - 4.0 * a * cc
            hit = (-b - np.sqrt(disc)) / (2.0 * a)
            t = np.where((disc >= 0) & (hit > 0) & (hit < t), hit, t)
    mm = np.where(np.isfinite(t), np.rint(t * 1000.0), 0.0)
    return np.where(mm < 65535, mm, 0).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--icp-iterations", type=int, default=50)
    a = ap.parse_args()
    vox = a.voxel
    K = tp.PinholeCameraIntrinsic(a.width, a.height, 0.95 * a.width, 0.95 * a.width, (a.width - 1) / 2.0, (a.height - 1) / 2.0)
    target_pose = np.eye(4)                      # the target camera is the world's frame
    source_pose = np.eye(4)                      # the planted pose: source camera -> target camera
    source_pose[:3, :3], source_pose[:3, 3] = rotation(np.radians(-3.0), np.radians(8.0)), [0.18, -0.04, 0.03]
    frames = [render_depth(K, source_pose), render_depth(K, target_pose)]

    t0 = time.perf_counter()
    src, dst = tp.create_point_cloud_from_depth_image_batch(frames, K, depth_scale=1000.0, depth_trunc=4.0)
    t1 = time.perf_counter()
    print("unprojection: %d x %d frames -> %d / %d points (one call, %.1f ms with the handle's creation)"
          % (a.width, a.height, len(src), len(dst), 1e3 * (t1 - t0)))
    A, B = (c.astype(np.float32) for c in tp.voxel_down_sample_batch([src, dst], vox))
    est = tp.FPFHEstimation()
    fa = est.computeFPFHFeatures(A, 2 * vox, 5 * vox)
    fb = est.computeFPFHFeatures(B, 2 * vox, 5 * vox)
    corr = tp.Matcher().calculateCorrespondences(A, B, fa, fb, False, True, False, 0.0)
    params = tp.RobustRegistrationSolver.Params(noise_bound=vox, cbar2=1.0, estimate_scaling=False,
                                                rotation_gnc_factor=1.4, rotation_max_iterations=10000,
                                                rotation_cost_threshold=1e-16)
    solver = tp.RobustRegistrationSolver(params)
    sol = solver.solve_correspondences(A, B, corr)
    print("%d / %d points after down-sampling, %d correspondences, max clique %d"
          % (len(A), len(B), len(corr), len(solver.getInlierMaxClique())))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = sol.rotation, sol.translation
    icp = tp.registration_icp(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64), vox, T,
                              tp.TransformationEstimationPointToPoint(), tp.ICPConvergenceCriteria(max_iteration=a.icp_iterations))

    def pose_error(M):
        cos = (np.trace(M[:3, :3].T @ source_pose[:3, :3]) - 1.0) / 2.0
        return np.degrees(np.arccos(min(1.0, max(-1.0, cos)))), np.linalg.norm(M[:3, 3] - source_pose[:3, 3])

    print("TEASER++ pose error: rotation %.4f deg, translation %.5f" % pose_error(T))
    print("ICP pose error: rotation %.4f deg, translation %.5f (fitness %.4f, rmse %.5f, %d iterations)"
          % (pose_error(icp.transformation) + (icp.fitness, icp.inlier_rmse, icp.iterations)))

    # the registered source in the target's camera: the estimated pose is the extrinsic of the source's own points
    seen = tp.project_to_depth_image(src, a.width, a.height, K, icp.transformation, depth_scale=1000.0, depth_max=4.0)
    target = frames[1].astype(np.float32)
    valid = target > 0
    covered = valid & (seen > 0)
    agree = covered & (np.abs(seen - target) < 1000.0 * vox)
    print("projection: %d of %d target pixels covered by the registered source; %d of them (%.1f %%) agree within a voxel; "
          "%.1f %% of all target pixels" % (int(covered.sum()), int(valid.sum()), int(agree.sum()),
                                            100.0 * agree.sum() / max(int(covered.sum()), 1),
                                            100.0 * agree.sum() / max(int(valid.sum()), 1)))


if __name__ == "__main__":
    main()
