#!/usr/bin/env python3
"""ISS keypoint detection on the MI355X: what it costs and what it buys the stages behind it.

  (a) compute_iss_keypoints on one config-5 down-sampled cloud (default parameters: automatic radii), and 64 jittered
      copies in one call against 64 single calls;
  (b) the numpy restatement (tests/keypoints_reference.py) on the same host and cloud -- the only baseline there is;
  (c) for the config-5 pair: the time of correspondences on all points against FPFH on all points + matching the
      keypoints' descriptor rows, the TEASER++ solve time behind each, the number of correspondences and the recovered
      pose error against the committed pose of tests/golden/config5_result_golden.json.

Every timing is a host clock around a call that ends in a device synchronise, after `--warmup` untimed calls, median
and spread of `--reps`.  Needs an MI355X: there is no CPU path.

    python scripts/bench_keypoints.py --reps 10 --warmup 2 --out profiles/keypoints/bench_keypoints.json"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
tp = importlib.import_module("teaser-plusplus_amd")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def pose_error(R, t, Rg, tg):
    c = np.clip((np.trace(Rg.T @ R) - 1) / 2, -1, 1)
    return dict(rotation_deg=float(np.degrees(np.arccos(c))), translation=float(np.linalg.norm(t - tg)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host-ref", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoints", "bench_keypoints.json"))
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_keypoints.py needs an MI355X")
    c5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    A, B, vox = c5["cloud_bin_0"].astype(np.float64), c5["cloud_bin_4"].astype(np.float64), float(c5["voxel_size"])
    out = dict(cloud_points=[len(A), len(B)], voxel=vox)

    # (a)
    rng = np.random.default_rng(1)
    copies = [A + 0.1 * vox * rng.standard_normal(A.shape) for _ in range(64)]
    ka = tp.compute_iss_keypoints(A)
    out["a"] = dict(keypoints=int(len(ka)),
                    one_cloud=timed(lambda: tp.compute_iss_keypoints(A), a.reps, a.warmup),
                    one_cloud_given_radii=timed(lambda: tp.compute_iss_keypoints(A, 6 * 0.6 * vox, 4 * 0.6 * vox), a.reps, a.warmup),
                    batch64_one_call=timed(lambda: tp.compute_iss_keypoints_batch(copies), a.reps, a.warmup),
                    batch64_single_calls=timed(lambda: [tp.compute_iss_keypoints(c) for c in copies], a.reps, a.warmup))
    # (b)
    if not a.no_host_ref:
        import keypoints_reference as RK
        t = time.perf_counter()
        ref = RK.iss_keypoints(A)
        out["b"] = dict(numpy_restatement_ms=1e3 * (time.perf_counter() - t),
                        mask_equal=bool(np.array_equal(np.flatnonzero(ref["keep"]), ka)))
    # (c)
    params = tp.RobustRegistrationSolver.Params(noise_bound=vox, cbar2=1.0, estimate_scaling=False,
                                                rotation_gnc_factor=1.4, rotation_max_iterations=10000,
                                                rotation_cost_threshold=1e-16)
    solver = tp.RobustRegistrationSolver(params)
    est = tp.FPFHEstimation()

    def front(iss):
        if not iss:
            return np.asarray(tp.correspondences_batch([A], [B], 2 * vox, 5 * vox)[0])
        fa, fb = est.computeFPFHFeatures(A, 2 * vox, 5 * vox), est.computeFPFHFeatures(B, 2 * vox, 5 * vox)
        k0, k1 = tp.compute_iss_keypoints_batch([A, B])
        c = np.asarray(tp.Matcher().calculateCorrespondences(A[k0], B[k1], fa[k0], fb[k1], False, True, False, 0.0, 0))
        return np.stack([k0[c[:, 0]], k1[c[:, 1]]], 1) if len(c) else np.zeros((0, 2), dtype=np.int64)

    gt_path = os.path.join(ROOT, "tests", "golden", "config5_result_golden.json")
    poses = {}
    out["c"] = {}
    for name, iss in (("without_iss", False), ("with_iss", True)):
        corr = front(iss)
        row = dict(correspondences=int(len(corr)), front_end=timed(lambda: front(iss), a.reps, a.warmup))
        if len(corr) >= 3:
            pairs = [tuple(r) for r in corr.tolist()]
            row["solve"] = timed(lambda: solver.solve_correspondences(A, B, pairs), a.reps, a.warmup)
            sol = solver.solve_correspondences(A, B, pairs)
            poses[name] = (np.array(sol.rotation), np.array(sol.translation))
        out["c"][name] = row
    g = json.load(open(gt_path))  # the committed TEASER++ pose of the pair
    ref_pose, against = (np.asarray(g["rotation"]).reshape(3, 3), np.asarray(g["translation"])), "tests/golden/config5_result_golden.json"
    out["c"]["pose_error_against"] = against
    for name, (R, t) in poses.items():
        if ref_pose is not None:
            out["c"][name]["pose_error"] = pose_error(R, t, ref_pose[0], ref_pose[1])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
