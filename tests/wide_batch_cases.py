"""The numpy restatements of the wide batches (320 problems per front-end), each computed once per process and shared
between tests/test_gpu_wide_batches.py, which compares the device with them, and tests/test_wide_batch_cases.py, which
runs the builders' assertions and times the restatements without a GPU.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import boundary_reference as RB
import dbscan_reference as RD
import fgr_reference as RF
import fpfh_o3d_reference as RH
import fps_reference as RP
import icp_colored_reference as RC
import information_reference as RI
import odometry_reference as RO
import plane_reference as PR
import posegraph_cases as PC
import ransac_reference as RR
import rgbd_reference as RG
import search_reference as RS

EDGE_OF = lambda b: (0, 63, 64, 65, 255, 256, 257, b - 1)  # noqa: E731  (the problems also called alone)
once = functools.lru_cache(maxsize=None)


def columns(w, keys):
    return zip(*[w[k] for k in keys])


# ---- plane segmentation ---------------------------------------------------------------------------------------------
PLANE_KEYS = ("clouds", "d", "ransac_n", "num_iterations", "probability", "seed")


@once
def plane():
    """(batch, per-problem trial records of the 70 trials, per-problem full results)."""
    w = PR.wide_batch()
    trials = [PR.trials(P, d, rn, seed, 0, it) for P, d, rn, it, _, seed in columns(w, PLANE_KEYS)]
    full = [PR.segment(*args) for args in columns(w, PLANE_KEYS)]
    return w, trials, full


# ---- RANSAC on correspondences --------------------------------------------------------------------------------------
RANSAC_KEYS = ("P", "Q", "corr", "r", "ransac_n", "max_iteration", "confidence", "seed", "s")


@once
def ransac():
    """(batch, per-problem RR.ransac)."""
    w = RR.wide_batch()
    return w, [RR.ransac(*args) for args in columns(w, RANSAC_KEYS)]


# ---- FGR ------------------------------------------------------------------------------------------------------------
@once
def fgr():
    """(problems, options, per problem (longdouble restatement, |T_f64 - T_longdouble|) of the full call, the same of
    the stage call's RF.WIDE_STAGE iterations)."""
    problems, options = RF.wide_batch()
    LD = np.longdouble

    def pair(P, Q, corr, o, n):
        ld = RF.fgr(P, Q, corr, dtype=LD, n=n, **o)
        f64 = RF.fgr(P, Q, corr, dtype=np.float64, n=n, **o)
        return ld, float(np.abs(f64["transformation"].astype(LD) - ld["transformation"]).max())

    full = [pair(P, Q, c, o, None) for (P, Q, c), o in zip(problems, options)]
    staged = [pair(P, Q, c, dict(o, iteration_number=max(o["iteration_number"], RF.WIDE_STAGE)), RF.WIDE_STAGE)
              for (P, Q, c), o in zip(problems, options)]
    return problems, options, full, staged


# ---- pose graphs ----------------------------------------------------------------------------------------------------
@once
def posegraph():
    """(names, {name: (float64 restatement, longdouble restatement)})."""
    names = PC.wide_batch()
    return names, {n: PC.reference(n) for n in sorted(set(names))}


# ---- information matrices -------------------------------------------------------------------------------------------
@once
def information():
    """(problems (P, Q, T, r), per-problem RI.information)."""
    w = RI.wide_batch()
    return w, [RI.information(P, Q, r, T) for P, Q, T, r in w]


# ---- colored ICP ----------------------------------------------------------------------------------------------------
COLOR_MAX_NN = (33, 64, 30)  # the second gradient call's max_nn, in turn: both list capacities in one launch


@once
def colored():
    """(scenes, gradients at max_nn 30, gradients at COLOR_MAX_NN in turn, RC.registration_icp with its margins)."""
    w = RC.wide_batch()
    g30 = [RC.color_gradients(s["target"], s["target_normals"], s["target_colors"], 2 * s["r"], 30) for s in w]
    gmix = [RC.color_gradients(s["target"], s["target_normals"], s["target_colors"], 2 * s["r"],
                               COLOR_MAX_NN[i % 3]) for i, s in enumerate(w)]
    reg = [RC.registration_icp(s["source"], s["target"], s["source_colors"], s["target_colors"], s["target_normals"],
                               s["r"], kernel=s["kernel"][0], k=s["kernel"][1], gradients=g,
                               max_iteration=RC.WIDE_ITERATIONS, margins=True) for s, g in zip(w, g30)]
    return w, g30, gmix, reg


def colored_margins_hold(reg):
    """The margins tests/test_icp_colored_reference.py asks of a scene before equal correspondence sets and iteration
    counts are a fair demand."""
    return all(r["margins"]["best_gap"] > 1e-7 and r["margins"]["radius_gap"] > 1e-7 and r["margins"]["stop_gap"] > 1e-9
               for r in reg)


# ---- two-cloud search -----------------------------------------------------------------------------------------------
@once
def search():
    """(batch, k-NN with k in turn, hybrid with max_nn <= 32, hybrid with max_nn up to 100, radius), each per problem."""
    w = RS.wide_batch()
    short = [min(k, 32) for k in w["k"]]
    knn = [RS.knn_search(P, Q, k) for P, Q, k in zip(w["data"], w["query"], w["k"])]
    hyb = [[RS.hybrid_search(P, Q, r, k) for P, Q, r, k in zip(w["data"], w["query"], w["hybrid_radius"], ks)]
           for ks in (short, w["k"])]
    rad = [RS.radius_search(P, Q, r) for P, Q, r in zip(w["data"], w["query"], w["radius"])]
    return w, knn, short, hyb[0], hyb[1], rad


# ---- FPFH (Open3D form) and boundary points -------------------------------------------------------------------------
BOUNDARY_ANGLES = (90.0, 45.0, 170.0)  # the angle thresholds of the boundary test, in turn


@once
def fpfh():
    """(batch, per-cloud (fpfh, spfh))."""
    w = RH.wide_batch()
    return w, [RH.compute_fpfh_feature(*c) for c in w]


@once
def boundary():
    """(batch, per-cloud (mask, max_gap, m))."""
    w = RH.wide_batch()
    return w, [RB.boundary_points(P, N, s, r, k, BOUNDARY_ANGLES[i % 3]) for i, (P, N, s, r, k) in enumerate(w)]


# ---- DBSCAN ---------------------------------------------------------------------------------------------------------
@once
def dbscan():
    """(clouds, eps, min_points, per-cloud (labels, counts, roots, n_clusters))."""
    clouds, eps, mp = RD.wide_batch()
    return clouds, eps, mp, [RD.dbscan(P, e, m) for P, e, m in zip(clouds, eps, mp)]


# ---- farthest-point down-sampling -----------------------------------------------------------------------------------
@once
def fps():
    """(clouds, K, start, per-cloud (index, sel_dist, final_dist))."""
    clouds, K, start = RP.wide_batch()
    return clouds, K, start, [RP.fps(P, k, s) for P, k, s in zip(clouds, K, start)]


# ---- RGB-D unprojection and projection ------------------------------------------------------------------------------
@once
def rgbd():
    """(frame case per problem, cloud case per problem, RG.unproject per case, RG.project per case)."""
    frames, clouds = RG.wide_batch()
    return (frames, clouds, [RG.unproject(d, c, f) for _, d, c, f in RG.unproject_cases()],
            [RG.project(P, C, cam) for _, P, C, cam in RG.project_cases()])


# ---- RGB-D odometry -------------------------------------------------------------------------------------------------
@once
def odometry():
    """(names, {name: RO.compute of the case})."""
    names = RO.wide_batch()
    return names, {n: RO.result(n) for n in sorted(set(names))}
