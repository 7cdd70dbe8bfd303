#!/usr/bin/env python3
"""Measures the batched ICP (teaser-plusplus_amd.registration_icp / registration_icp_batch), point-to-point and
point-to-plane side by side in the same run, and prints ONE JSON object.  Point-to-point, at the top level:
  single      one config-5 refinement (tests/golden/config5_clouds.npz, TEASER++ seed, r = voxel, max_iteration 100)
  batch64     64 config-5 problems (perturbed seeds) in one call, against the same 64 as sequential single calls
  dense       the jittered ~250 k-point upsampling of config 5 (one problem), with an estimate of the bytes a
              correspondence pass moves (source read + write, match write, candidate coordinates + indices)
  host_ref    the numpy + cKDTree restatement (tests/icp_reference.py) on the same host, single-threaded Python
Point-to-plane, under "plane" (target normals of the committed fixture tests/golden/icp_plane_golden.npz): the same
three workloads for the L2 kernel (single_l2) and Tukey with k = voxel / 2 (single, batch64, dense), each with its
per-iteration cost relative to point-to-point in this run.
Wall-clock medians over --reps calls after --warmup calls (every call is synchronous); ms_min / ms_max give the spread
of the repeats.  --method point skips the point-to-plane part (the form that also runs on a build without it).  Usage:
    python scripts/bench_icp.py [--reps 20] [--warmup 3] [--no-host-ref] [--method both|point|plane]"""
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
import icp_reference as R  # noqa: E402

tp = importlib.import_module("teaser-plusplus_amd")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    timed.spread = dict(ms_min=1e3 * min(ts), ms_max=1e3 * max(ts), reps=reps)
    return float(np.median(ts)), out


def perturbed(init, k, rng):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = np.deg2rad(rng.uniform(0, 3))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = rng.normal(0, 0.02, 3)
    return T @ init


def candidate_visits(X, Q, r):
    """Target points in the 27 cells (edge r) around each source point, summed: the candidates one pass reads."""
    o = Q.min(axis=0)
    cq = np.floor((Q - o) / r).astype(np.int64)
    keys, counts = np.unique(cq, axis=0, return_counts=True)
    table = {tuple(k): int(c) for k, c in zip(keys, counts)}
    cs, mult = np.unique(np.floor((X - o) / r).astype(np.int64), axis=0, return_counts=True)
    total = 0
    for c, m in zip(cs, mult):
        s = 0
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    s += table.get((c[0] + dx, c[1] + dy, c[2] + dz), 0)
        total += s * int(m)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host-ref", action="store_true")
    ap.add_argument("--method", choices=["both", "point", "plane"], default="both")
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_icp.py needs an MI355X")
    P, Q, r, init = R.config5_problem()
    crit = tp.ICPConvergenceCriteria(max_iteration=100)
    res = {"workload": "ICP, config-5 pair (%d / %d points), r = voxel = %.4f, max_iteration 100"
                       % (len(P), len(Q), r)}

    rng = np.random.default_rng(2024)
    inits = [perturbed(init, k, rng) for k in range(64)]
    drng = np.random.default_rng(5)
    A = np.repeat(P, 48, axis=0) + drng.normal(0, 0.01, size=(48 * len(P), 3))
    B = np.repeat(Q, 50, axis=0) + drng.normal(0, 0.01, size=(50 * len(Q), 3))

    def workloads(est, N):
        """single / batch64 / dense for one estimation method (None: point-to-point, through the original calls)."""
        kw = {} if est is None else dict(estimation_method=est, target_normals=N)
        out = {}
        t, o = timed(lambda: tp.registration_icp(P, Q, r, init, criteria=crit, **kw), a.reps, a.warmup)
        out["single"] = dict(ms=1e3 * t, iterations=o.iterations, us_per_iteration=1e6 * t / max(o.iterations, 1),
                             fitness=o.fitness, inlier_rmse=o.inlier_rmse, correspondences=len(o.correspondence_set),
                             **timed.spread)
        bkw = {} if est is None else dict(estimation_methods=est, target_normals=[N] * 64)
        srcs, dsts = [P] * 64, [Q] * 64
        tb, ob = timed(lambda: tp.registration_icp_batch(srcs, dsts, r, inits, crit, **bkw), a.reps, a.warmup)
        sb = timed.spread
        ts, _ = timed(lambda: [tp.registration_icp(P, Q, r, T, criteria=crit, **kw) for T in inits],
                      max(a.reps // 4, 3), 1)
        its = [x.iterations for x in ob]
        out["batch64"] = dict(batch_ms=1e3 * tb, sequential_ms=1e3 * ts, speedup=ts / tb,
                              iterations_min=min(its), iterations_max=max(its), iterations_mean=float(np.mean(its)),
                              us_per_batch_iteration=1e6 * tb / max(its), **sb)
        dkw = {} if est is None else dict(estimation_method=est, target_normals=np.repeat(N, 50, axis=0))
        td, od = timed(lambda: tp.registration_icp(A, B, r, init, criteria=crit, **dkw), max(a.reps // 4, 3), 1)
        cand = candidate_visits(R.apply(od.transformation, A), B, r)
        per_pass = len(A) * (48 + 4 + (24 if est is not None else 0)) + cand * 28  # + one gathered normal per point
        out["dense"] = dict(points=[len(A), len(B)], ms=1e3 * td, iterations=od.iterations,
                            us_per_iteration=1e6 * td / max(od.iterations, 1), fitness=od.fitness,
                            candidates_per_pass=cand, bytes_per_pass_estimate=per_pass,
                            effective_GBps=per_pass * (od.iterations + 1) / td / 1e9, **timed.spread)
        return out

    t = None
    if a.method in ("both", "point"):
        res.update(workloads(None, None))
        t = res["single"]["ms"] / 1e3
    if a.method in ("both", "plane"):
        g = np.load(os.path.join(ROOT, "tests", "golden", "icp_plane_golden.npz"))
        N = g["target_normals"]
        pl = workloads(tp.TransformationEstimationPointToPlane(tp.TukeyLoss(float(g["tukey_k"]))), N)
        pl["kernel"] = "Tukey, k = %.4f" % float(g["tukey_k"])
        tl, ol = timed(lambda: tp.registration_icp(P, Q, r, init, tp.TransformationEstimationPointToPlane(), crit,
                                                   target_normals=N), a.reps, a.warmup)
        pl["single_l2"] = dict(ms=1e3 * tl, iterations=ol.iterations, us_per_iteration=1e6 * tl / max(ol.iterations, 1),
                               fitness=ol.fitness, inlier_rmse=ol.inlier_rmse, **timed.spread)
        if "single" in res:
            pl["per_iteration_vs_point_to_point"] = dict(
                single=pl["single"]["us_per_iteration"] / res["single"]["us_per_iteration"],
                single_l2=pl["single_l2"]["us_per_iteration"] / res["single"]["us_per_iteration"],
                dense=pl["dense"]["us_per_iteration"] / res["dense"]["us_per_iteration"],
                batch64=pl["batch64"]["us_per_batch_iteration"] / res["batch64"]["us_per_batch_iteration"])
        res["plane"] = pl

    if not a.no_host_ref and t is not None:
        t0 = time.perf_counter()
        ro = R.registration_icp(P, Q, r, init, max_iteration=100)
        th = time.perf_counter() - t0
        cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
        res["host_ref"] = dict(ms=1e3 * th, iterations=ro["iterations"], python_threads=1, cores_available=cores)
        res["host_ref"]["speedup_single"] = th / t
    print(json.dumps(res))


if __name__ == "__main__":
    main()
