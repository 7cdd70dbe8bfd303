#!/usr/bin/env python3
"""The workflow of the reference's examples/teaser_python_fpfh_icp (helpers.py:9-60, without Open3D): two
clouds -> voxel down-sampling (example.py:19-20, Open3D's voxel_down_sample) -> FPFH features -> mutual
nearest-neighbour correspondences -> TEASER++ registration -> optional DRS certificate -> optional ICP refinement
(example.py:66-71: registration_icp seeded with the TEASER++ pose, max_correspondence_distance = voxel), everything
on the MI355X.  Usage:

    python examples/teaser_python_fpfh.py [src.ply dst.ply] [--voxel 0.05] [--certify] [--icp [--icp-iterations 100]]
                                          [--remove-plane D [--plane-seed N]] [--cluster EPS,MIN_POINTS]
                                          [--icp-plane [--icp-kernel tukey --icp-kernel-k K]]
                                          [--icp-plane-normals hybrid:R:K|knn:K]
                                          [--icp-gicp [--gicp-radius R --gicp-max-nn K]] [--batch K]
                                          [--knn K [--no-mutual]] [--tuple-scale S [--tuple-seed N]]
                                          [--iss [--iss-radii RS,RN]] [--fps K]
                                          [--ransac [--ransac-iterations N --ransac-seed N]]
                                          [--fgr [--fgr-tuple-test --fgr-seed N]] [--open3d-fpfh]
                                          [--drop-boundary ANGLE]

--open3d-fpfh computes the descriptors the way Open3D's global-registration scripts do, in place of the PCL form: the
extract_fpfh helper's estimate_normals(KDTreeSearchParamHybrid(2 voxels, 30)) and compute_fpfh_feature(
KDTreeSearchParamHybrid(5 voxels, 100)) in FP64, both clouds (with --batch all 2 K clouds) in ONE call on the GPU, the
normals never leaving the device in between.  Everything downstream -- the matcher, --knn, --ransac, --fgr, --batch --
takes these rows as it takes the PCL form's; --icp-plane then refines on these normals.

--drop-boundary ANGLE removes the boundary points of BOTH clouds (Open3D's compute_boundary_points on the GPU: the
normals' own neighbourhood KDTreeSearchParamHybrid(2 voxels, 30), the normals estimated inside the same call, angle
threshold ANGLE degrees) after every other filter and before the descriptors, and prints how many points and
correspondences remain beside the count of the same run without it.  The clouds are partial scans: along their rim the
neighbourhood is half empty, and normals and descriptors are least reliable there.  Off by default.

--remove-plane D drops the dominant plane (Open3D's segment_plane on the GPU: distance_threshold D, ransac_n 3, 1 000
iterations, seeded by --plane-seed) from BOTH clouds after down-sampling and before FPFH, in one batched call, and
prints each plane and the share of points removed.  A floor or a road holds a large part of a scan, its descriptors are
all alike, and it lets ICP slide along it.  Off by default.

--cluster EPS,MIN_POINTS splits each cloud into objects (Open3D's cluster_dbscan on the GPU, both clouds in one call)
after --remove-plane and --remove-outliers and before FPFH, prints the number of clusters and of noise points per cloud,
and keeps the most populous cluster of each (ties go to the smaller label): what is left of a scene once its floor is
gone is a handful of objects, and the largest one is what gets registered.  Off by default.

--ransac runs Open3D's registration_ransac_based_on_correspondence on the GPU on the SAME correspondences the TEASER++
solver got (max_correspondence_distance = 1.5 voxels, the edge-length checker at 0.9 and the distance checker at 1.5
voxels, as Open3D's global-registration tutorial sets them) and prints its pose, fitness, RMSE and trial counts beside
TEASER++'s, with the rotation and translation difference between the two.  --ransac-iterations is RANSAC-1K / 10K's N.

--fgr runs Open3D's registration_fgr_based_on_correspondence (Fast Global Registration) on the GPU on the SAME
correspondences (maximum_correspondence_distance = 0.5 voxels, as Open3D's global-registration tutorial sets it, the
other options at their defaults) and prints its pose, fitness and RMSE beside TEASER++'s in the same way.
--fgr-tuple-test first passes the pairs through the tuple test (tuple_scale 0.95, seeded by --fgr-seed).

--iss detects ISS keypoints (Open3D's compute_iss_keypoints) in both down-sampled clouds on the GPU and matches only
them: FPFH is still computed on the whole clouds (its neighbourhoods need every point), the descriptor rows at the
keypoints go to the matcher, and the returned pairs are mapped back to cloud indices.  --iss-radii RS,RN gives the
salient and the suppression radius; the default takes 6 and 4 times each cloud's resolution, like Open3D.

--cloud-distance prints, after the registration, the mean and the largest distance from the registered source's
points to their nearest target points (Open3D's compute_point_cloud_distance: a k = 1 search between the two clouds on
the GPU) and how many of them lie closer than the voxel size -- the overlap of the pair.

--fps K matches only K well-spread points of each down-sampled cloud (Open3D's farthest_point_down_sample on the GPU,
both clouds in one call), applied where --iss is applied: the descriptors are computed on the whole cloud and kept at the
K samples, and the returned pairs are mapped back to cloud indices.  A cloud of fewer than K points keeps all of them.
Unlike a voxel size or the ISS radii, K fixes the number of keypoints, and with it the solver's cost, in advance; with
--batch every pair gets exactly min(K, n) keypoints per cloud, all clouds sampled in one call.  --fps and --iss together
are an error.

--knn K matches every point with its K nearest descriptors (helpers.py:19-43, find_knn_cpu(feat0, feat1, knn=K)) in
place of the single mutual nearest neighbour: more putative correspondences for the solver, on the GPU as well.  Only
pairs that are among each other's K nearest are kept unless --no-mutual is given.

--tuple-scale S applies the matcher's tuple constraint (matcher.cc:223-283) to the correspondences, with or without
--knn: a correspondence survives when it occurs in a random triple whose side lengths agree within the factor S in
both clouds.  --tuple-seed N makes the draw reproducible; 0 (the default) seeds from the clock like the reference.

--icp-plane refines with point-to-plane ICP instead, on the target normals the FPFH stage already computed
(rows PCL leaves non-finite, below 3 neighbours, set to zero: they contribute nothing), optionally with a robust kernel.

--batch K registers K perturbed copies of the pair (each moved by a seeded random rigid transform and jittered by a
tenth of a voxel) through the four batched stages, one call each: voxel_down_sample_batch -> correspondences_batch ->
solve_batch -> registration_icp_batch, and prints the wall time of every stage.

Without file arguments it runs BASELINE config 5 from tests/golden/config5_clouds.npz (the 3DMatch pair
cloud_bin_0 / cloud_bin_4 after a 0.05 voxel grid); with two PLY files (ASCII or binary little-endian, float x y z)
it down-samples them on the GPU first, giving exactly that fixture for the tutorial's two clouds."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
tp = importlib.import_module("teaser-plusplus_amd")


def read_ply_xyz(path):
    with open(path, "rb") as f:
        header = []
        while True:
            line = f.readline().decode("ascii", "replace").strip()
            header.append(line)
            if line == "end_header":
                break
        n = int([h.split()[2] for h in header if h.startswith("element vertex")][0])
        props = [h.split()[2] for h in header if h.startswith("property")]
        if any(h.startswith("format ascii") for h in header):
            data = np.loadtxt(f, max_rows=n, dtype=np.float64)
            return data[:, [props.index("x"), props.index("y"), props.index("z")]].astype(np.float32)
        dt = np.dtype([(p, "<f4") for p in props])  # float properties only
        data = np.frombuffer(f.read(n * dt.itemsize), dtype=dt, count=n)
        return np.stack([data["x"], data["y"], data["z"]], axis=1).astype(np.float32)


def parse_outliers(text):
    """--remove-outliers NB,RATIO -> (nb_neighbors, std_ratio), or None when the option is absent."""
    if not text:
        return None
    nb, ratio = text.split(",")
    return int(nb), float(ratio)


def open3d_fpfh(clouds, vox, return_normals=False):
    """Open3D's extract_fpfh for every cloud, one call: normals Hybrid(2 v, 30), features Hybrid(5 v, 100)."""
    return tp.compute_fpfh_feature_batch([np.asarray(c, dtype=np.float64) for c in clouds], None,
                                         tp.KDTreeSearchParamHybrid(5 * vox, 100),
                                         normal_search=tp.KDTreeSearchParamHybrid(2 * vox, 30),
                                         return_normals=return_normals)


def run_batch(A, B, vox, K, icp_iterations, knn=0, mutual=True, tuple_scale=0.0, tuple_seed=0, outliers=None, fps=0,
              o3d=False):
    """K perturbed copies of the pair (A, B) through the batched stages, one call per stage."""
    rng = np.random.default_rng(555)
    srcs, dsts = [], []
    for _ in range(K):
        q = rng.standard_normal(4)
        w, x, y, z = q / np.linalg.norm(q)
        Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                       [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        srcs.append((A + 0.1 * vox * rng.standard_normal(A.shape) - rng.uniform(-1, 1, 3)) @ Rm)
        dsts.append(B + 0.1 * vox * rng.standard_normal(B.shape))
    params = tp.RobustRegistrationSolver.Params(noise_bound=vox, cbar2=1.0, estimate_scaling=False,
                                                rotation_gnc_factor=1.4, rotation_max_iterations=10000,
                                                rotation_cost_threshold=1e-16)               # helpers.py:45-60
    solver = tp.RobustRegistrationSolver(params)
    crit = tp.ICPConvergenceCriteria(max_iteration=icp_iterations)
    for timed in (False, True):  # the first pass creates the handles and grows the arenas
        t0 = time.perf_counter()
        down = tp.voxel_down_sample_batch(srcs + dsts, vox)
        n_down = sum(map(len, down))
        t1 = time.perf_counter()
        if outliers:  # one call cleans all 2 K clouds
            down = [c for c, _ in tp.remove_statistical_outlier_batch(down, outliers[0], outliers[1])]
        t_clean = time.perf_counter() - t1
        t1 = time.perf_counter()
        sp, dp = down[:K], down[K:]
        if fps or o3d:  # descriptors on the whole clouds, matching at min(fps, n) well-spread samples of each
            feats = open3d_fpfh(down, vox) if o3d else tp.compute_fpfh_batch(down, 2 * vox, 5 * vox)
            if fps:
                keys = tp.farthest_point_down_sample_batch(down, [min(fps, len(c)) for c in down])
            else:
                keys = [np.arange(len(c)) for c in down]
            fk = [f[k] for f, k in zip(feats, keys)]
            if knn:
                corr = tp.match_features_knn_batch(fk[:K], fk[K:], knn, mutual)
            else:
                corr = tp.match_features_batch(fk[:K], fk[K:])
            if tuple_scale:
                corr = tp.tuple_test_batch([c[k] for c, k in zip(sp, keys[:K])], [c[k] for c, k in zip(dp, keys[K:])],
                                           corr, tuple_scale, tuple_seed)
            corr = [np.stack([keys[k][c[:, 0]], keys[K + k][c[:, 1]]], axis=1) for k, c in enumerate(corr)]
        elif knn:
            corr = tp.correspondences_knn_batch(sp, dp, 2 * vox, 5 * vox, knn, mutual, tuple_scale=tuple_scale,
                                                tuple_seed=tuple_seed)
        else:
            corr = tp.correspondences_batch(sp, dp, 2 * vox, 5 * vox, tuple_scale=tuple_scale,
                                            tuple_seed=tuple_seed)   # helpers.py:9-43 for every pair
        t2 = time.perf_counter()
        if min(map(len, corr)) < 3:
            sys.exit("pair %d has %d correspondences: nothing to register" % (int(np.argmin([len(c) for c in corr])),
                                                                              min(map(len, corr))))
        sols = solver.solve_batch([sp[k][corr[k][:, 0]].T for k in range(K)], [dp[k][corr[k][:, 1]].T for k in range(K)])
        t3 = time.perf_counter()
        inits = []
        for sol in sols:
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = sol.rotation, sol.translation
            inits.append(T)
        icp = tp.registration_icp_batch(sp, dp, vox, inits, crit)
        t4 = time.perf_counter()
    print("%d pairs: %d .. %d points after down-sampling, %d .. %d correspondences"
          % (K, min(map(len, down)), max(map(len, down)), min(map(len, corr)), max(map(len, corr))))
    if fps:
        print("farthest-point samples: %d .. %d per cloud (--fps %d, one call for all %d clouds)"
              % (min(map(len, keys)), max(map(len, keys)), fps, 2 * K))
    if outliers:
        print("statistical outlier removal (nb_neighbors %d, std_ratio %g): %d points went from %d clouds, %.1f ms"
              % (outliers[0], outliers[1], n_down - sum(map(len, down)), 2 * K, 1e3 * t_clean))
    print("down-sampling %.1f ms, front-end %.1f ms, registration %.1f ms, ICP %.1f ms (one call each, second pass)"
          % (1e3 * (t1 - t_clean - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (t4 - t3)))
    print("ICP fitness %.4f .. %.4f, rmse %.4f .. %.4f" % (min(r.fitness for r in icp), max(r.fitness for r in icp),
                                                         min(r.inlier_rmse for r in icp), max(r.inlier_rmse for r in icp)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("clouds", nargs="*")
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--certify", action="store_true")
    ap.add_argument("--icp", action="store_true", help="refine the TEASER++ pose with point-to-point ICP")
    ap.add_argument("--icp-iterations", type=int, default=100)
    ap.add_argument("--icp-plane", action="store_true",
                    help="refine the TEASER++ pose with point-to-plane ICP on the FPFH stage's target normals")
    ap.add_argument("--icp-plane-normals", default=None, metavar="hybrid:R:K|knn:K",
                    help="refine with point-to-plane ICP on target normals estimated from the target cloud on the "
                         "GPU: the K nearest neighbours inside radius R, or the K nearest")
    ap.add_argument("--icp-gicp", action="store_true",
                    help="refine with Generalized ICP instead, on covariances estimated on the GPU from both clouds")
    ap.add_argument("--gicp-radius", type=float, default=None, help="covariance search radius (default: 2 voxels)")
    ap.add_argument("--gicp-max-nn", type=int, default=20)
    ap.add_argument("--icp-kernel", choices=["l2", "huber", "cauchy", "gm", "tukey"], default="l2")
    ap.add_argument("--icp-kernel-k", type=float, default=None, help="kernel parameter (default: the voxel size)")
    ap.add_argument("--batch", type=int, default=0, metavar="K",
                    help="register K perturbed copies of the pair through the batched stages")
    ap.add_argument("--knn", type=int, default=0, metavar="K",
                    help="match every point with its K nearest descriptors (1 .. 16) instead of the nearest one")
    ap.add_argument("--no-mutual", action="store_true", help="with --knn: keep one-directional matches too")
    ap.add_argument("--tuple-scale", type=float, default=0.0, metavar="S",
                    help="apply the matcher's tuple constraint with this factor (0: off, the reference uses 0.95)")
    ap.add_argument("--tuple-seed", type=int, default=0, metavar="N", help="seed of the tuple test (0: the clock)")
    ap.add_argument("--remove-outliers", default="", metavar="NB,RATIO",
                    help="clean both clouds after down-sampling with statistical outlier removal on the GPU "
                         "(Open3D's remove_statistical_outlier(NB, RATIO), e.g. 20,2.0)")
    ap.add_argument("--iss", action="store_true",
                    help="match only the ISS keypoints of both clouds (detected on the GPU); single pair only")
    ap.add_argument("--iss-radii", default="", metavar="RS,RN",
                    help="with --iss: salient and non-maximum-suppression radius (default: 6 and 4 resolutions)")
    ap.add_argument("--fps", type=int, default=0, metavar="K",
                    help="match only K farthest-point samples of each cloud (selected on the GPU)")
    ap.add_argument("--ransac", action="store_true",
                    help="also run RANSAC on the same correspondences (on the GPU) and print it beside TEASER++")
    ap.add_argument("--ransac-iterations", type=int, default=100000, metavar="N")
    ap.add_argument("--ransac-seed", type=int, default=1, metavar="N", help="seed of the trials (0: the clock)")
    ap.add_argument("--fgr", action="store_true",
                    help="also run Fast Global Registration on the same correspondences (on the GPU)")
    ap.add_argument("--fgr-tuple-test", action="store_true", help="with --fgr: Open3D's tuple test on the pairs first")
    ap.add_argument("--fgr-seed", type=int, default=1, metavar="N", help="seed of the tuple test (0: the clock)")
    ap.add_argument("--remove-plane", type=float, default=0.0, metavar="D",
                    help="drop the dominant plane (segment_plane, distance threshold D) from both clouds before FPFH")
    ap.add_argument("--plane-seed", type=int, default=1, metavar="N", help="seed of the plane trials (0: the clock)")
    ap.add_argument("--cloud-distance", action="store_true",
                    help="print the mean and the largest source-to-target distance after registration (nearest-"
                         "neighbour search between the two clouds on the GPU); single pair only")
    ap.add_argument("--open3d-fpfh", action="store_true",
                    help="Open3D's descriptors (estimate_normals Hybrid(2 v, 30) + compute_fpfh_feature Hybrid(5 v, "
                         "100), FP64, one call on the GPU) in place of the PCL form")
    ap.add_argument("--drop-boundary", type=float, default=None, metavar="ANGLE",
                    help="drop the boundary points of both clouds (compute_boundary_points on the GPU, normals estimated "
                         "in the call, Hybrid(2 v, 30), angle threshold in degrees, e.g. 90) before the descriptors")
    ap.add_argument("--cluster", default="", metavar="EPS,MIN_POINTS",
                    help="keep the most populous DBSCAN cluster of each cloud (cluster_dbscan on the GPU, e.g. 0.1,10)")
    a = ap.parse_args()
    if a.remove_plane > 0 and a.batch > 0:
        ap.error("--remove-plane serves a single pair: it cannot be combined with --batch")
    if a.cluster and a.batch > 0:
        ap.error("--cluster serves a single pair: it cannot be combined with --batch")
    if a.drop_boundary is not None and a.batch > 0:
        ap.error("--drop-boundary serves a single pair: it cannot be combined with --batch")
    if a.fps < 0:
        ap.error("--fps takes a number of samples")
    if a.fps and a.iss:
        ap.error("--fps and --iss both choose the keypoints: give one of them")
    if a.iss and a.batch > 0:
        ap.error("--iss registers a single pair: it cannot be combined with --batch")
    if a.cloud_distance and a.batch > 0:
        ap.error("--cloud-distance measures a single pair: it cannot be combined with --batch")
    if a.batch > 0:
        if len(a.clouds) == 2:
            A, B = (read_ply_xyz(c).astype(np.float64) for c in a.clouds)
        else:
            c5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
            A, B, a.voxel = c5["cloud_bin_0"].astype(np.float64), c5["cloud_bin_4"].astype(np.float64), float(c5["voxel_size"])
        return run_batch(A, B, a.voxel, a.batch, a.icp_iterations, a.knn, not a.no_mutual, a.tuple_scale, a.tuple_seed,
                         parse_outliers(a.remove_outliers), a.fps, a.open3d_fpfh)
    t_ds = None
    if len(a.clouds) == 2:
        raw = [read_ply_xyz(c).astype(np.float64) for c in a.clouds]
        tp.voxel_down_sample(raw[0][:1], a.voxel)  # handle creation stays out of the timing
        t = time.perf_counter()
        A, B = (ds.astype(np.float32) for ds in tp.voxel_down_sample_batch(raw, a.voxel))   # example.py:19-20
        t_ds = time.perf_counter() - t
        print("voxel down-sampling: %d / %d -> %d / %d points" % (len(raw[0]), len(raw[1]), len(A), len(B)))
    else:
        c5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
        A, B, a.voxel = c5["cloud_bin_0"], c5["cloud_bin_4"], float(c5["voxel_size"])
    vox = a.voxel
    if a.remove_plane > 0:  # the floor or the road floods the matcher with look-alike descriptors: take it out first
        t = time.perf_counter()
        found = tp.segment_plane_batch([A, B], a.remove_plane, 3, 1000, 0.99999999, a.plane_seed)
        t_plane = time.perf_counter() - t
        kept = []
        for name, cloud, r in (("source", A, found[0]), ("target", B, found[1])):
            print("dominant plane of the %s: %s, %d of %d points (%.1f %%) removed after %d trials"
                  % (name, np.array2string(r.plane_model, precision=5), len(r.inliers), len(cloud),
                     100.0 * len(r.inliers) / max(len(cloud), 1), r.trials))
            kept.append(cloud[r.mask == 0])
        print("plane segmentation of both clouds: %.1f ms (one call)" % (1e3 * t_plane))
        A, B = kept
    outliers = parse_outliers(a.remove_outliers)
    if outliers:
        t = time.perf_counter()
        (A2, ia), (B2, ib) = tp.remove_statistical_outlier_batch([A, B], outliers[0], outliers[1])
        print("statistical outlier removal (nb_neighbors %d, std_ratio %g): %d / %d points went, %d / %d stay (%.1f ms)"
              % (outliers[0], outliers[1], len(A) - len(ia), len(B) - len(ib), len(ia), len(ib),
                 1e3 * (time.perf_counter() - t)))
        A, B = A2.astype(A.dtype), B2.astype(B.dtype)
    if a.cluster:  # what is left of the scene falls into objects: register the largest one
        eps, min_points = a.cluster.split(",")
        t = time.perf_counter()
        labels, n_clusters = tp.cluster_dbscan_batch([A, B], float(eps), int(min_points))
        t_cluster = time.perf_counter() - t
        kept = []
        for name, cloud, lab, c in (("source", A, labels[0], int(n_clusters[0])), ("target", B, labels[1], int(n_clusters[1]))):
            print("DBSCAN clusters of the %s: %d clusters, %d of %d points are noise" % (name, c, int((lab < 0).sum()), len(cloud)))
            if c == 0:
                sys.exit("no cluster in the %s: nothing to register" % name)
            largest = int(np.argmax(np.bincount(lab[lab >= 0], minlength=c)))  # argmax: the first of equal sizes
            kept.append(cloud[lab == largest])
            print("  kept cluster %d: %d points" % (largest, len(kept[-1])))
        print("clustering of both clouds: %.1f ms (one call)" % (1e3 * t_cluster))
        A, B = kept

    def descriptors(A, B, quiet=False):
        if a.open3d_fpfh:  # Open3D's extract_fpfh for both clouds in one call
            (fa, _), (fb, nb) = open3d_fpfh([A, B], vox, return_normals=True)
            if not quiet:
                print("Open3D-form FPFH: %d + %d rows of %d float64, normals and features in one call" % (len(fa), len(fb), fa.shape[1]))
            return fa, fb, nb
        est = tp.FPFHEstimation()
        fa = est.computeFPFHFeatures(A, 2 * vox, 5 * vox)   # helpers.py:9-18: radii 2 and 5 voxels
        fb = est.computeFPFHFeatures(B, 2 * vox, 5 * vox)
        return fa, fb, est.getNormals()   # the target's normals: point-to-plane ICP refines on them

    def match(A, B, fa, fb):
        if a.knn:
            corr = tp.match_features_knn(fa, fb, a.knn, not a.no_mutual)   # helpers.py:19-43
            if a.tuple_scale:
                corr = tp.tuple_test_batch([A], [B], [corr], a.tuple_scale, a.tuple_seed)[0]
            return [tuple(r) for r in corr.tolist()]
        return tp.Matcher().calculateCorrespondences(A, B, fa, fb, False, True, bool(a.tuple_scale), a.tuple_scale,
                                                     a.tuple_seed)   # helpers.py:27-43

    if a.drop_boundary is not None:  # the rim of a partial scan: half-empty neighbourhoods, unreliable descriptors
        fa, fb, _ = descriptors(A, B, quiet=True)
        without = len(match(A, B, fa, fb))
        t = time.perf_counter()
        search = tp.KDTreeSearchParamHybrid(2 * vox, 30)   # the normals' own neighbourhood
        rim = tp.compute_boundary_points_batch([np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)], None,
                                               search, a.drop_boundary, normal_search=search)
        t_rim = time.perf_counter() - t
        print("boundary points (Hybrid(%g, 30), angle threshold %g degrees): %d of %d / %d of %d points dropped, "
              "%d / %d remain (%.1f ms, one call)" % (2 * vox, a.drop_boundary, rim[0].n_boundary, len(A),
                                                      rim[1].n_boundary, len(B), len(A) - rim[0].n_boundary,
                                                      len(B) - rim[1].n_boundary, 1e3 * t_rim))
        A, B = A[~rim[0].mask], B[~rim[1].mask]
    t0 = time.perf_counter()
    fa, fb, nb = descriptors(A, B)
    full = (A, B)
    if a.iss:  # the matcher sees the keypoints only; `keys` maps its pairs back to cloud indices
        rs, rn = (float(v) for v in a.iss_radii.split(",")) if a.iss_radii else (0.0, 0.0)
        t = time.perf_counter()
        keys = tp.compute_iss_keypoints_batch([A, B], rs, rn)
        print("ISS keypoints: %d of %d / %d of %d points (%.1f ms)" % (len(keys[0]), len(A), len(keys[1]), len(B),
                                                                       1e3 * (time.perf_counter() - t)))
        if min(map(len, keys)) < 3:
            sys.exit("fewer than 3 keypoints in a cloud: nothing to match")
        A, B, fa, fb = A[keys[0]], B[keys[1]], fa[keys[0]], fb[keys[1]]
    if a.fps:  # the same, at a number of well-spread points fixed in advance
        t = time.perf_counter()
        keys = tp.farthest_point_down_sample_batch([A, B], [min(a.fps, len(A)), min(a.fps, len(B))])
        print("farthest-point samples: %d of %d / %d of %d points (%.1f ms)"
              % (len(keys[0]), len(A), len(keys[1]), len(B), 1e3 * (time.perf_counter() - t)))
        if min(map(len, keys)) < 3:
            sys.exit("fewer than 3 samples in a cloud: nothing to match")
        A, B, fa, fb = A[keys[0]], B[keys[1]], fa[keys[0]], fb[keys[1]]
    corr = match(A, B, fa, fb)
    if a.iss or a.fps:
        corr = [(int(keys[0][i]), int(keys[1][j])) for i, j in corr]
        A, B = full
    t1 = time.perf_counter()
    params = tp.RobustRegistrationSolver.Params(noise_bound=vox, cbar2=1.0, estimate_scaling=False,
                                                rotation_gnc_factor=1.4, rotation_max_iterations=10000,
                                                rotation_cost_threshold=1e-16)               # helpers.py:45-60
    solver = tp.RobustRegistrationSolver(params)
    sol = solver.solve_correspondences(A, B, corr)
    t2 = time.perf_counter()
    print("%d / %d points, %d correspondences, max clique %d" % (len(A), len(B), len(corr),
                                                                 len(solver.getInlierMaxClique())))
    if a.drop_boundary is not None:
        print("without --drop-boundary: %d correspondences; with it: %d; solution valid: %s"
              % (without, len(corr), bool(sol.valid)))
    print("%sfront-end %.1f ms, registration %.1f ms" % ("" if t_ds is None else "down-sampling %.1f ms, " % (1e3 * t_ds),
                                                       1e3 * (t1 - t0), 1e3 * (t2 - t1)))
    print("R =\n%s\nt = %s" % (sol.rotation, sol.translation))
    if a.cloud_distance:  # Open3D's source.compute_point_cloud_distance(target) on the registered source
        moved = np.asarray(A, dtype=np.float64) @ np.asarray(sol.rotation).T + np.asarray(sol.translation)
        t3 = time.perf_counter()
        dist = tp.compute_point_cloud_distance(moved, np.asarray(B, dtype=np.float64))
        t4 = time.perf_counter()
        print("source-to-target distance after registration: mean %.6f max %.6f, %d of %d source points closer than "
              "the voxel size (%.1f ms, %d queries served by the scan of the whole target)"
              % (dist.mean(), dist.max(), int((dist < vox).sum()), len(dist), 1e3 * (t4 - t3),
                 tp.get_icp_option("knn_fallbacks")))
    if a.ransac:
        P, Q = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        pairs = np.array(corr, dtype=np.int32).reshape(-1, 2)
        checkers = [tp.CorrespondenceCheckerBasedOnEdgeLength(0.9), tp.CorrespondenceCheckerBasedOnDistance(1.5 * vox)]
        crit = tp.RANSACConvergenceCriteria(a.ransac_iterations, 0.999)
        tp.registration_ransac_based_on_correspondence(P[:3], Q[:3], [[0, 0]] * 3, vox, seed=1,
                                                       criteria=tp.RANSACConvergenceCriteria(1, 0.999))  # the handle
        t3 = time.perf_counter()
        rs = tp.registration_ransac_based_on_correspondence(P, Q, pairs, 1.5 * vox, None, 3, checkers, crit,
                                                            seed=a.ransac_seed)
        t4 = time.perf_counter()
        Rr, tr = rs.transformation[:3, :3], rs.transformation[:3, 3]
        cos = min(1.0, max(-1.0, (np.trace(Rr.T @ sol.rotation) - 1.0) / 2.0))
        print("RANSAC on the same %d correspondences: %d of %d trials valid, best trial %d, %.1f ms"
              % (len(pairs), rs.valid_trials, rs.trials, rs.best_trial, 1e3 * (t4 - t3)))
        print("RANSAC fitness %.6f rmse %.6f inliers %d" % (rs.fitness, rs.inlier_rmse, len(rs.correspondence_set)))
        print("R_ransac =\n%s\nt_ransac = %s" % (Rr, tr))
        print("RANSAC against TEASER++: rotation %.4g rad, translation %.4g" % (np.arccos(cos),
                                                                               np.linalg.norm(tr - sol.translation)))
    if a.fgr:
        P, Q = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        pairs = np.array(corr, dtype=np.int32).reshape(-1, 2)
        opt = tp.FastGlobalRegistrationOption(maximum_correspondence_distance=0.5 * vox, tuple_test=a.fgr_tuple_test,
                                              seed=a.fgr_seed)
        tp.registration_fgr_based_on_correspondence(P[:3], Q[:3], [[0, 0]] * 3, opt)  # the handles
        t3 = time.perf_counter()
        fg = tp.registration_fgr_based_on_correspondence(P, Q, pairs, opt)
        t4 = time.perf_counter()
        Rf, tf = fg.transformation[:3, :3], fg.transformation[:3, 3]
        cos = min(1.0, max(-1.0, (np.trace(Rf.T @ sol.rotation) - 1.0) / 2.0))
        print("FGR on %d of the same %d correspondences: %d iterations, %d failed solves, final mu %.4g, %.1f ms"
              % (fg.fgr["n_corr"], len(pairs), fg.fgr["iterations"], fg.fgr["failed_solves"], fg.fgr["final_mu"],
                 1e3 * (t4 - t3)))
        print("FGR fitness %.6f rmse %.6f inliers %d" % (fg.fitness, fg.inlier_rmse, len(fg.correspondence_set)))
        print("R_fgr =\n%s\nt_fgr = %s" % (Rf, tf))
        print("FGR against TEASER++: rotation %.4g rad, translation %.4g" % (np.arccos(cos),
                                                                            np.linalg.norm(tf - sol.translation)))
    if a.certify:
        c = np.array(corr)
        inl = np.zeros(len(c), dtype=bool)
        inl[solver.getInlierMaxClique()] = True
        cert = tp.DRSCertifier(noise_bound=vox, cbar2=1.0, max_iterations=100)
        # the certifier works on the translation-free measurements of the clique's correspondences
        src = A[c[:, 0]].astype(np.float64).T
        dst = B[c[:, 1]].astype(np.float64).T - sol.translation.reshape(3, 1)
        res = cert.certify(sol.rotation, src[:, inl], dst[:, inl], np.ones(int(inl.sum())))
        print(res)
    if a.icp:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = sol.rotation, sol.translation
        P, Q = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        crit = tp.ICPConvergenceCriteria(max_iteration=a.icp_iterations)
        before = tp.registration_icp(P, Q, vox, T, criteria=tp.ICPConvergenceCriteria(max_iteration=0))
        t3 = time.perf_counter()
        icp = tp.registration_icp(P, Q, vox, T, tp.TransformationEstimationPointToPoint(), crit)   # example.py:66-71
        t4 = time.perf_counter()
        print("ICP before: fitness %.6f rmse %.6f" % (before.fitness, before.inlier_rmse))
        print("ICP after:  fitness %.6f rmse %.6f iterations %d (%.2f ms)" % (icp.fitness, icp.inlier_rmse,
                                                                              icp.iterations, 1e3 * (t4 - t3)))
        print("T_icp =\n%s" % icp.transformation)
    if a.icp_plane:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = sol.rotation, sol.translation
        P, Q = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        N = np.asarray(nb, dtype=np.float64)
        N[~np.isfinite(N).all(axis=1)] = 0.0
        k = a.icp_kernel_k if a.icp_kernel_k is not None else vox
        kernel = dict(l2=tp.L2Loss, huber=lambda: tp.HuberLoss(k), cauchy=lambda: tp.CauchyLoss(k),
                      gm=lambda: tp.GMLoss(k), tukey=lambda: tp.TukeyLoss(k))[a.icp_kernel]()
        crit = tp.ICPConvergenceCriteria(max_iteration=a.icp_iterations)
        before = tp.registration_icp(P, Q, vox, T, criteria=tp.ICPConvergenceCriteria(max_iteration=0))
        t3 = time.perf_counter()
        icp = tp.registration_icp(P, Q, vox, T, tp.TransformationEstimationPointToPlane(kernel), crit,
                                  target_normals=N)
        t4 = time.perf_counter()
        print("point-to-plane, kernel %r" % (kernel,))
        print("ICP before: fitness %.6f rmse %.6f" % (before.fitness, before.inlier_rmse))
        print("ICP after:  fitness %.6f rmse %.6f iterations %d (%.2f ms)" % (icp.fitness, icp.inlier_rmse,
                                                                              icp.iterations, 1e3 * (t4 - t3)))
        print("T_icp =\n%s" % icp.transformation)
    if a.icp_plane_normals:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = sol.rotation, sol.translation
        P, Q = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        kind, *rest = a.icp_plane_normals.split(":")
        if kind == "hybrid" and len(rest) == 2:
            search = tp.KDTreeSearchParamHybrid(float(rest[0]), int(rest[1]))
        elif kind == "knn" and len(rest) == 1:
            search = tp.KDTreeSearchParamKNN(int(rest[0]))
        else:
            raise SystemExit("--icp-plane-normals takes hybrid:R:K or knn:K")
        k = a.icp_kernel_k if a.icp_kernel_k is not None else vox
        kernel = dict(l2=tp.L2Loss, huber=lambda: tp.HuberLoss(k), cauchy=lambda: tp.CauchyLoss(k),
                      gm=lambda: tp.GMLoss(k), tukey=lambda: tp.TukeyLoss(k))[a.icp_kernel]()
        crit = tp.ICPConvergenceCriteria(max_iteration=a.icp_iterations)
        before = tp.registration_icp(P, Q, vox, T, criteria=tp.ICPConvergenceCriteria(max_iteration=0))
        t3 = time.perf_counter()
        icp = tp.registration_icp(P, Q, vox, T, tp.TransformationEstimationPointToPlane(kernel), crit,
                                  target_normals=search)  # the normals are estimated on the device and stay there
        t4 = time.perf_counter()
        print("point-to-plane on self-estimated normals (%r), kernel %r" % (search, kernel))
        print("ICP before: fitness %.6f rmse %.6f" % (before.fitness, before.inlier_rmse))
        print("ICP after:  fitness %.6f rmse %.6f iterations %d (%.2f ms)" % (icp.fitness, icp.inlier_rmse,
                                                                              icp.iterations, 1e3 * (t4 - t3)))
        print("T_icp =\n%s" % icp.transformation)
    if a.icp_gicp:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = sol.rotation, sol.translation
        P, Q = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        radius = a.gicp_radius if a.gicp_radius is not None else 2 * vox
        crit = tp.ICPConvergenceCriteria(max_iteration=a.icp_iterations)
        before = tp.registration_icp(P, Q, vox, T, criteria=tp.ICPConvergenceCriteria(max_iteration=0))
        t3 = time.perf_counter()
        Cs, Ct = tp.estimate_covariances_batch([P, Q], radius, a.gicp_max_nn)
        t4 = time.perf_counter()
        icp = tp.registration_generalized_icp(P, Q, vox, T, tp.TransformationEstimationForGeneralizedICP(), crit,
                                              source_covariances=Cs, target_covariances=Ct)
        t5 = time.perf_counter()
        print("Generalized ICP, covariances from radius %g, max_nn %d (%.2f ms)" % (radius, a.gicp_max_nn,
                                                                                    1e3 * (t4 - t3)))
        print("ICP before: fitness %.6f rmse %.6f" % (before.fitness, before.inlier_rmse))
        print("ICP after:  fitness %.6f rmse %.6f iterations %d (%.2f ms)" % (icp.fitness, icp.inlier_rmse,
                                                                              icp.iterations, 1e3 * (t5 - t4)))
        print("T_icp =\n%s" % icp.transformation)


if __name__ == "__main__":
    main()
