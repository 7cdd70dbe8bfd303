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
Generalized ICP, under "gicp" (covariances estimated on the GPU at radius = 2 voxel, max_nn = 20): the same three
workloads, beside point-to-plane L2 on all three from the same run ("plane_l2") and the per-iteration ratio against it,
the iterations to convergence of the three methods on config 5, and "covariances": the estimation time per cloud for
the config-5 pair (each cloud alone, both in one call, 64 pairs in one call) and the dense pair.
Colored ICP, with --colored alone (nothing else runs): under "colored" the textured scene of
tests/icp_colored_reference.py scaled up (144 x 144 targets, 15 000 sources, r = 0.04) and config 5 with a synthetic
texture (intensity 0.5 + 0.2 sin 4x + 0.2 cos 3y of the world position, the fixture's target normals), each alone and
x 64 in one call: ms per call and per iteration beside point-to-plane L2 on the same pairs in the same run, the pose
errors on the scene, and the gradient estimation alone.  The object is also written to
profiles/icp_colored/bench_icp_colored.json.
Wall-clock medians over --reps calls after --warmup calls (every call is synchronous); ms_min / ms_max give the spread
of the repeats.  --method point skips the other parts (the form that also runs on a build without them); both = point + plane.  Usage:
    python scripts/bench_icp.py [--reps 20] [--warmup 3] [--no-host-ref] [--method all|both|point|plane|gicp]
    python scripts/bench_icp.py --colored [--reps 20] [--warmup 3]"""
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


def colored_part(a):
    """The "colored" object: Colored ICP beside point-to-plane L2 on the same pairs."""
    import icp_colored_reference as RC
    crit = tp.ICPConvergenceCriteria(max_iteration=100)

    def texture(X):
        i = 0.5 + 0.2 * np.sin(4 * X[:, 0]) + 0.2 * np.cos(3 * X[:, 1])
        return np.stack([i, i, i], 1)

    def pair(name, P, Q, N, Cs, Ct, r, init, T_true=None):
        est, pl = tp.TransformationEstimationForColoredICP(), tp.TransformationEstimationPointToPlane()
        out = {"points": [len(P), len(Q)], "r": r}
        for label, b in (("single", 1), ("batch64", 64)):
            kw = dict(estimation_methods=est, target_normals=[N] * b, source_colors=[Cs] * b, target_colors=[Ct] * b)
            reps = a.reps if b == 1 else max(a.reps // 4, 3)
            tc, oc = timed(lambda: tp.registration_icp_batch([P] * b, [Q] * b, r, init, crit, **kw), reps, a.warmup)
            sc = timed.spread
            tpl, op = timed(lambda: tp.registration_icp_batch([P] * b, [Q] * b, r, init, crit, estimation_methods=pl,
                                                              target_normals=[N] * b), reps, a.warmup)
            row = dict(colored_ms=1e3 * tc, colored_iterations=oc[0].iterations,
                       colored_us_per_iteration=1e6 * tc / max(oc[0].iterations, 1), colored_fitness=oc[0].fitness,
                       plane_ms=1e3 * tpl, plane_iterations=op[0].iterations,
                       plane_us_per_iteration=1e6 * tpl / max(op[0].iterations, 1), plane_spread=timed.spread, **sc)
            if T_true is not None:
                row["colored_pose_error"] = float(np.linalg.norm(oc[0].transformation - T_true))
                row["plane_pose_error"] = float(np.linalg.norm(op[0].transformation - T_true))
            out[label] = row
        tg, _ = timed(lambda: tp.estimate_color_gradients(Q, N, Ct, 2 * r), a.reps, a.warmup)
        out["gradients_alone"] = dict(ms=1e3 * tg, radius=2 * r, max_nn=30, **timed.spread)
        return name, out

    res = {}
    s = RC.scene(seed=0, n_src=15000, grid=144)
    k, v = pair("scene", s["source"], s["target"], s["target_normals"], s["source_colors"], s["target_colors"], 0.04,
                np.eye(4), s["T_true"])
    res[k] = v
    P, Q, r, init = R.config5_problem()
    N = np.load(os.path.join(ROOT, "tests", "golden", "icp_plane_golden.npz"))["target_normals"]
    k, v = pair("config5", P, Q, N, texture(R.apply(init, P)), texture(Q), r, init)
    res[k] = v
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host-ref", action="store_true")
    ap.add_argument("--method", choices=["all", "both", "point", "plane", "gicp"], default="all")
    ap.add_argument("--colored", action="store_true", help="Colored ICP beside point-to-plane, nothing else")
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_icp.py needs an MI355X")
    if a.colored:
        res = {"workload": "Colored ICP beside point-to-plane L2, max_iteration 100", "colored": colored_part(a)}
        out_dir = os.path.join(ROOT, "profiles", "icp_colored")
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "bench_icp_colored.json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    P, Q, r, init = R.config5_problem()
    crit = tp.ICPConvergenceCriteria(max_iteration=100)
    res = {"workload": "ICP, config-5 pair (%d / %d points), r = voxel = %.4f, max_iteration 100"
                       % (len(P), len(Q), r)}

    rng = np.random.default_rng(2024)
    inits = [perturbed(init, k, rng) for k in range(64)]
    drng = np.random.default_rng(5)
    A = np.repeat(P, 48, axis=0) + drng.normal(0, 0.01, size=(48 * len(P), 3))
    B = np.repeat(Q, 50, axis=0) + drng.normal(0, 0.01, size=(50 * len(Q), 3))

    def workloads(est, N=None, cov=None, dense_cov=None):
        """single / batch64 / dense for one estimation method (None: point-to-point, through the original calls).
        N: target normals of a point-to-plane method; cov / dense_cov: (source, target) covariances of a Generalized-ICP
        method for the config-5 pair and for the dense pair."""
        kw, bkw, dkw, gathered = {}, {}, {}, 0  # gathered: bytes read once per matched point after the search
        if cov is not None:
            kw = dict(estimation_method=est, source_covariances=cov[0], target_covariances=cov[1])
            bkw = dict(estimation_methods=est, source_covariances=[cov[0]] * 64, target_covariances=[cov[1]] * 64)
            dkw = dict(estimation_method=est, source_covariances=dense_cov[0], target_covariances=dense_cov[1])
            gathered = 96
        elif est is not None:
            kw = dict(estimation_method=est, target_normals=N)
            bkw = dict(estimation_methods=est, target_normals=[N] * 64)
            dkw = dict(estimation_method=est, target_normals=np.repeat(N, 50, axis=0))
            gathered = 24
        out = {}
        t, o = timed(lambda: tp.registration_icp(P, Q, r, init, criteria=crit, **kw), a.reps, a.warmup)
        out["single"] = dict(ms=1e3 * t, iterations=o.iterations, us_per_iteration=1e6 * t / max(o.iterations, 1),
                             fitness=o.fitness, inlier_rmse=o.inlier_rmse, correspondences=len(o.correspondence_set),
                             **timed.spread)
        srcs, dsts = [P] * 64, [Q] * 64
        tb, ob = timed(lambda: tp.registration_icp_batch(srcs, dsts, r, inits, crit, **bkw), a.reps, a.warmup)
        sb = timed.spread
        ts, _ = timed(lambda: [tp.registration_icp(P, Q, r, T, criteria=crit, **kw) for T in inits],
                      max(a.reps // 4, 3), 1)
        its = [x.iterations for x in ob]
        out["batch64"] = dict(batch_ms=1e3 * tb, sequential_ms=1e3 * ts, speedup=ts / tb,
                              iterations_min=min(its), iterations_max=max(its), iterations_mean=float(np.mean(its)),
                              us_per_batch_iteration=1e6 * tb / max(its), **sb)
        td, od = timed(lambda: tp.registration_icp(A, B, r, init, criteria=crit, **dkw), max(a.reps // 4, 3), 1)
        cand = candidate_visits(R.apply(od.transformation, A), B, r)
        per_pass = len(A) * (48 + 4 + gathered) + cand * 28
        out["dense"] = dict(points=[len(A), len(B)], ms=1e3 * td, iterations=od.iterations,
                            us_per_iteration=1e6 * td / max(od.iterations, 1), fitness=od.fitness,
                            candidates_per_pass=cand, bytes_per_pass_estimate=per_pass,
                            effective_GBps=per_pass * (od.iterations + 1) / td / 1e9, **timed.spread)
        return out

    t = None
    if a.method in ("all", "both", "point"):
        res.update(workloads(None, None))
        t = res["single"]["ms"] / 1e3
    if a.method in ("all", "both", "plane"):
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

    if a.method in ("all", "gicp"):
        radius, max_nn = 2 * r, 20
        cv = {}
        tc, cov = timed(lambda: tp.estimate_covariances_batch([P, Q], radius, max_nn), a.reps, a.warmup)
        cv["config5_pair_one_call"] = dict(ms=1e3 * tc, ms_per_cloud=1e3 * tc / 2, **timed.spread)
        ts_, _ = timed(lambda: tp.estimate_covariances(P, radius, max_nn), a.reps, a.warmup)
        cv["config5_source_alone"] = dict(ms=1e3 * ts_, points=len(P), **timed.spread)
        tt_, _ = timed(lambda: tp.estimate_covariances(Q, radius, max_nn), a.reps, a.warmup)
        cv["config5_target_alone"] = dict(ms=1e3 * tt_, points=len(Q), **timed.spread)
        t64, _ = timed(lambda: tp.estimate_covariances_batch([P, Q] * 64, radius, max_nn), max(a.reps // 4, 3), 1)
        cv["config5_64_pairs_one_call"] = dict(ms=1e3 * t64, ms_per_cloud=1e3 * t64 / 128, **timed.spread)
        tdc, dense_cov = timed(lambda: tp.estimate_covariances_batch([A, B], radius, max_nn), 3, 1)
        cv["dense_pair_one_call"] = dict(ms=1e3 * tdc, ms_per_cloud=1e3 * tdc / 2, points=[len(A), len(B)],
                                         **timed.spread)
        gi = workloads(tp.TransformationEstimationForGeneralizedICP(), cov=cov, dense_cov=dense_cov)
        gi["covariances"] = dict(radius=radius, max_nn=max_nn, **cv)
        N = np.load(os.path.join(ROOT, "tests", "golden", "icp_plane_golden.npz"))["target_normals"]
        l2 = workloads(tp.TransformationEstimationPointToPlane(), N)
        gi["plane_l2"] = l2
        gi["per_iteration_vs_plane_l2"] = dict(
            single=gi["single"]["us_per_iteration"] / l2["single"]["us_per_iteration"],
            dense=gi["dense"]["us_per_iteration"] / l2["dense"]["us_per_iteration"],
            batch64=gi["batch64"]["us_per_batch_iteration"] / l2["batch64"]["us_per_batch_iteration"])
        gi["iterations_config5"] = dict(gicp=gi["single"]["iterations"], plane_l2=l2["single"]["iterations"],
                                        point=res["single"]["iterations"] if "single" in res else None)
        res["gicp"] = gi

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
