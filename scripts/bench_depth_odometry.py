#!/usr/bin/env python3
"""Depth odometry (compute_depth_odometry_batch on the ICP handle) on the MI355X beside RGB-D odometry with the hybrid
term on the same frames, and one tracked frame against a TSDF model.

  (1) one 640 x 480 pair per call (uint16 depth, the default options: at most 18 iterations on three levels);
  (2) 64 such pairs (consecutive frames of the trajectory of examples/teaser_python_odometry.py, eight frames eight times
      over) in ONE call against 64 calls; the two must give the same bits;
  (3) beside each, in the same process and on the same frames, compute_rgbd_odometry_batch with the hybrid term and its
      own defaults (35 iterations);
  (4) the preprocessing stage alone;
  (5) one tracked frame (track_frame_to_model: ray cast of the depth map, the copy back, the upload, depth odometry) on
      the 512-voxel scene of scripts/bench_tsdf.py, dense and scalable, with the ray cast and the odometry of the same
      frame timed alone, so that what the copies and the host's work between them take is the remainder.

Call times are a host clock around a Python call that ends in a device synchronise, after `--warmup` untimed calls:
median, minimum and maximum of `--reps` (at least nine), all in one process.  Kernel time comes from a run of its own:
`--profile-workload one_call` (or `pair`, `rgbd_one_call`) runs the calls and writes nothing; `rocprofv3 --kernel-trace
--stats` is pointed at it, and its kernel_stats.csv is kept beside the JSON.  Needs an MI355X: there is no CPU path.

    python scripts/bench_depth_odometry.py --reps 9 --warmup 1 --out profiles/depth_odometry/bench_depth_odometry.json"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
tp = importlib.import_module("teaser-plusplus_amd")
ex = importlib.import_module("teaser_python_odometry")
fusion = importlib.import_module("teaser_python_tsdf")

W, H, PAIRS, FRAMES, MODEL_R, MODEL_FRAMES = 640, 480, 64, 9, 512, 16
DEPTH_MAX = 6.0


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def tracked_frame(scalable, reps, warmup):
    """One frame tracked against the model of 16 frames of the TSDF benchmark's scene; its parts timed alone."""
    K, depths, ext = fusion.scene_frames(W, H, MODEL_FRAMES)
    length, R, trunc, origin = fusion.volume_settings(MODEL_R)
    vol = (tp.ScalableTSDFVolume(length / R, trunc, tp.TSDFVolumeColorType.NoColor) if scalable
           else tp.UniformTSDFVolume(length, R, trunc, tp.TSDFVolumeColorType.NoColor, origin))
    option = tp.DepthOdometryOption(depth_max=DEPTH_MAX)
    with vol:
        vol.integrate_batch(depths[:-1], K, ext[:-1], None, 1000.0, DEPTH_MAX)
        init = np.linalg.inv(ext[-2])           # the pose of the frame before
        frame = depths[-1]
        tr = tp.track_frame_to_model(vol, frame, K, init, option, weight_threshold=3.0)
        res = dict(scalable=bool(scalable), R=MODEL_R, success=bool(tr.success), iterations=tr.result.iterations,
                   fitness=tr.result.fitness, inlier_rmse=tr.result.inlier_rmse, model_pixels=int((tr.model_depth > 0).sum()))
        e = ext[-1] @ tr.camera_to_world          # the true world-to-camera of the frame times its tracked pose
        res["rotation_error_deg"] = float(np.degrees(np.arccos(min(1.0, max(-1.0, (np.trace(e[:3, :3]) - 1.0) / 2.0)))))
        res["translation_error_m"] = float(np.linalg.norm(e[:3, 3]))
        res["tracked_frame"] = timed(lambda: tp.track_frame_to_model(vol, frame, K, init, option, weight_threshold=3.0), reps, warmup)
        res["ray_cast_depth_only"] = timed(lambda: vol.ray_cast_batch(K, [ext[-2]], W, H, depth_min=0.1, depth_max=DEPTH_MAX, weight_threshold=3.0,
                                                                      vertex_map=False, normal_map=False, color=False), reps, warmup)
        metres = frame.astype(np.float32) / np.float32(1000.0)
        res["odometry_alone"] = timed(lambda: tp.compute_depth_odometry(metres, tr.model_depth, K, None, option), reps, warmup)
    res["image_bytes_down_and_up"] = 4 * W * H * 3   # the model map down, the model map and the frame up
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-workload", choices=["one_call", "pair", "rgbd_one_call"], default=None)
    ap.add_argument("--skip-tracking", action="store_true")
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_depth_odometry.py needs an MI355X: no HIP device visible")
    K, poses, depths, paints = ex.sequence(W, H, FRAMES)
    rep = PAIRS // (FRAMES - 1)
    src, tgt = depths[:-1] * rep, depths[1:] * rep
    truth = [ex.true_motion(poses, k) for k in range(FRAMES - 1)] * rep
    rgbd = [tp.RGBDImage.create_from_color_and_depth(c, d, depth_scale=1000.0, depth_trunc=DEPTH_MAX) for c, d in zip(paints, depths)]
    rsrc, rtgt = rgbd[:-1] * rep, rgbd[1:] * rep
    option, roption = tp.DepthOdometryOption(depth_max=DEPTH_MAX), tp.OdometryOption(depth_max=DEPTH_MAX)

    def one_call(n=PAIRS):
        return tp.compute_depth_odometry_batch(src[:n], tgt[:n], K, option=option)

    def many_calls():
        return [tp.compute_depth_odometry_batch(src[k:k + 1], tgt[k:k + 1], K, option=option)[0] for k in range(PAIRS)]

    def rgbd_one_call(n=PAIRS):
        return tp.compute_rgbd_odometry_batch(rsrc[:n], rtgt[:n], K, option=roption)

    if a.profile_workload:
        for _ in range(3):
            if a.profile_workload == "rgbd_one_call":
                rgbd_one_call()
            else:
                one_call(PAIRS if a.profile_workload == "one_call" else 1)
        return
    batch, single = one_call(), many_calls()
    same = all(x.success == y.success and x.count == y.count and x.transformation.tobytes() == y.transformation.tobytes()
               and x.information.tobytes() == y.information.tobytes() for x, y in zip(batch, single))
    errs = [ex.pose_error(r.transformation, t) for r, t in zip(batch, truth)]
    rerrs = [ex.pose_error(r.transformation, t) for r, t in zip(rgbd_one_call(FRAMES - 1), truth)]
    its = [c if isinstance(c, int) else c.max_iteration for c in option.criteria]
    out = dict(workload=dict(width=W, height=H, pairs=PAIRS, iterations=its, launches_per_call=len(its) + 2 + 2 * sum(its) + 2,
                             rgbd_launches_per_call=3 * 3 + 4 + 3 * 35 + 3),
               same_bits_one_call_and_64_calls=bool(same), successes=int(sum(r.success for r in batch)),
               executed_iterations=[int(r.iterations) for r in batch[:FRAMES - 1]],
               correspondences=[int(r.count) for r in batch[:FRAMES - 1]],
               max_rotation_error_deg=float(max(e[0] for e in errs)), max_translation_error_m=float(max(e[1] for e in errs)),
               rgbd_hybrid_max_rotation_error_deg=float(max(e[0] for e in rerrs)),
               rgbd_hybrid_max_translation_error_m=float(max(e[1] for e in rerrs)))
    out["one_pair_per_call"] = timed(lambda: one_call(1), a.reps, a.warmup)
    out["one_call_64_pairs"] = timed(one_call, a.reps, a.warmup)
    out["calls_64"] = timed(many_calls, a.reps, a.warmup)
    out["pyramid_one_pair"] = timed(lambda: tp.depth_odometry_pyramid_batch(src[:1], tgt[:1], K, option=option), a.reps, a.warmup)
    out["rgbd_hybrid_one_pair_per_call"] = timed(lambda: rgbd_one_call(1), a.reps, a.warmup)
    out["rgbd_hybrid_one_call_64_pairs"] = timed(rgbd_one_call, a.reps, a.warmup)
    for key in ("one_call_64_pairs", "calls_64", "rgbd_hybrid_one_call_64_pairs"):
        out[key]["ms_per_pair"] = out[key]["median_ms"] / PAIRS
    out["batch_speedup"] = out["calls_64"]["median_ms"] / out["one_call_64_pairs"]["median_ms"]
    if not a.skip_tracking:
        out["tracking"] = [tracked_frame(False, a.reps, a.warmup), tracked_frame(True, a.reps, a.warmup)]
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
