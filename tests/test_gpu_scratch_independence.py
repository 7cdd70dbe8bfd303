"""No call's result depends on what its scratch buffers held.

Every handle but the solver's keeps grow-only device buffers and staging memory between its calls (csrc/host_common.h:
DevBuf, HostBuf), many of them shared by several front-ends.  A kernel that reads a byte its own call never wrote passes
every other test of the suite: fresh memory reads as zero, and a repeated call finds the leavings of an identical call.
Here the contents of scratch are an input.  teaser_hip_<kind>_fill_scratch (DIAGNOSTIC, include/teaser_hip.h) sets every
byte of every scratch and staging buffer of a handle, up to its capacity, to one value; each test

  1  warms the handle: the front-end's largest case, then the calls of step 3 once, so that no buffer has to grow later;
  2  fills the scratch and asserts that bytes were filled;
  3  runs the front-end's small cases, each alone, and a mixed batch where it has one, and compares every result with the
     numpy restatement through the front-end's own runner and checker (imported from its GPU test file: this file has
     no tolerance of its own -- where a front-end's comparison is written inside one of its tests and not as a function,
     the same expressions stand here with the bars of that test);
  4  fills again and asserts the same number of bytes: no buffer grew, so step 3 ran inside filled memory;
  5  asserts that the results of step 3 are the same bytes under every fill value run so far (_seen).

The fill values: 0x00 (what fresh memory gives), 0xFF (the value the key images and DBSCAN's labels must start from: it
would hide a missing 0xFF fill as fresh memory hides a missing zero-fill) and 0x3F (int32 1 061 109 567, double about
4.8e-4: plausible garbage that neither all-zeros nor NaN / -1 imitates).  DESIGN.md section 36 lists, buffer by buffer,
what initialises every word a kernel reads before it writes; that table was written from the host code before these
tests first ran on a device.  It found no word without an initialiser, and on the MI355X every front-end then passed
under all three fills at the first run: no product code changed but the fill entries.  (That a missing initialiser
fails here was checked once with a library built without the zero-fill of the projection's hit counters, an output
that is never an index: the projection tests and both of its order tests failed on n_hit.)

The second part needs no fill: for each pair (A, B) of front-ends of the ICP handle that share a buffer, A large, B
small, A small, B large on the one cached handle, every result against its restatement -- the order dependence that a
suite which runs one file at a time never exercises."""
import functools
import importlib
import os

import numpy as np
import pytest

import dbscan_reference as RD
import fps_reference as RFP
import icp_colored_reference as RC
import icp_gicp_reference as RGI
import icp_reference as RI0
import information_reference as RIN
import normals_reference as RN
import odometry_reference as ROD
import plane_reference as PR
import posegraph_cases as PC
import posegraph_reference as PGR
import ransac_reference as RR
import search_reference as RS
import tsdf_mesh_reference as TM
import tsdf_raycast_reference as TR
import tsdf_reference as T
import tuple_test_reference as RT
import voxel_reference as RV
import test_gpu_boundary as bd
import test_gpu_dbscan as db
import test_gpu_features_batch as fb
import test_gpu_features_knn as fk
import test_gpu_fgr as fg
import test_gpu_fpfh_o3d as fp
import test_gpu_fps as fpsm
import test_gpu_icp_colored as col
import test_gpu_icp_gicp as gi
import test_gpu_icp_step as step
import test_gpu_keypoints as kp
import test_gpu_normals as nm
import test_gpu_odometry as od
import test_gpu_outlier as ol
import test_gpu_plane as pl
import test_gpu_posegraph as pg
import test_gpu_ransac as rs
import test_gpu_rgbd as rg
import test_gpu_search as se
import test_gpu_tsdf as ts
import test_gpu_tsdf_mesh as tmesh
import test_gpu_tsdf_raycast as tray
import test_gpu_tuple_test as tt
import test_gpu_voxel as vx
from icp_colored_cases import scene, scene_gradients
from information_reference import grid_pair
from oracle import features as F
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")

FILLS = (0x00, 0xFF, 0x3F)
fills = pytest.mark.parametrize("fill", FILLS, ids=["0x00", "0xFF", "0x3F"])
_seen = {}  # front-end -> {fill value: the bytes of its step-3 results}
memo = functools.lru_cache(maxsize=None)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def blob(x):
    """Every number of a result as bytes, in a fixed order."""
    if x is None:
        return b"none"
    if isinstance(x, dict):
        return [(k, blob(x[k])) for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [blob(v) for v in x]
    if hasattr(x, "__dict__"):
        return blob({k: v for k, v in vars(x).items() if not k.startswith("_")})
    return np.asarray(x).tobytes()


def fill_of(kind):
    return lambda byte: tp.fill_scratch(kind, byte)


def independent(front, fill, filler, warm, calls):
    """Steps 1 .. 5 of the module's docstring.  calls() runs and CHECKS the small cases and returns their results."""
    warm()
    calls()
    filled = filler(fill)
    assert filled > 0, front
    got = blob(calls())
    again = filler(fill)
    assert again == filled, "%s: a buffer grew during the calls (%d -> %d bytes): the warm-up is too small" % (front, filled, again)
    seen = _seen.setdefault(front, {})
    seen[fill] = got
    for other, b in seen.items():
        assert b == got, "%s: the results under fill 0x%02X and 0x%02X differ" % (front, other, fill)


class ring_caps:
    """Runs its body at knn_ring_cap 4 (the ring walk and its worklist) and 0 (every query by the whole-cloud scan)."""

    def __iter__(self):
        before = tp.get_icp_option("knn_ring_cap")
        try:
            for cap in (4, 0):
                tp.set_icp_option("knn_ring_cap", cap)
                yield cap
        finally:
            tp.set_icp_option("knn_ring_cap", before)


def test_fill_scratch_refuses_a_byte_outside_0_to_255_and_names_the_kinds():
    for byte in (-1, 256):
        with pytest.raises(tp.TeaserHipError, match="byte must lie in 0..255"):
            tp.fill_scratch("icp", byte)
    with pytest.raises(ValueError):
        tp.fill_scratch("solver", 0)
    for kind in tp.SCRATCH_KINDS:
        assert tp.fill_scratch(kind, 0) >= 0


# ---- the ICP handle: the three estimation methods, one step at the sums' block edges (tests/test_gpu_icp_step.py) ------
def icp_fields(r):
    return (r.transformation, r.fitness, r.inlier_rmse, r.iterations, r.correspondence_set)


def icp_step_large(name):
    step.check_unique(name, step.run(step.case(name)))


def icp_step_small(prefix):
    names = [prefix + "_%d" % n for n in (255, 256, 257)]
    alone = [step.run(step.case(n)) for n in names]
    for n, out in zip(names, alone):
        step.check_unique(n, out)
    cs = [step.case(n) for n in names]
    batch = tp.registration_icp_batch([c["P"] for c in cs], [c["Q"] for c in cs], [c["r"] for c in cs],
                                      np.array([c["init"] for c in cs]), step.ONE,
                                      estimation_methods=[step.estimation(c) for c in cs],
                                      target_normals=[c["N"] for c in cs], source_covariances=[c["Cs"] for c in cs],
                                      target_covariances=[c["Ct"] for c in cs])
    for n, got, one in zip(names, batch, alone):
        assert blob(icp_fields(got)) == blob(icp_fields(one)), n
    return [icp_fields(r) for r in alone]


@fills
def test_point_to_point_icp(fill):
    independent("point_to_point", fill, fill_of("icp"), lambda: icp_step_large("gpt_65793"), lambda: icp_step_small("gpt"))


@fills
def test_point_to_plane_icp(fill):
    independent("point_to_plane", fill, fill_of("icp"), lambda: icp_step_large("gpl_65793"), lambda: icp_step_small("gpl"))


@memo
def covariance_reference(max_nn):
    """The slab lattice of tests/test_gpu_icp_gicp.py with its restatement and the points its comparison leaves out."""
    X = gi.slab_lattice()
    radius = 0.25 * np.sqrt(2.5)
    ref, _, _, _, lam = RGI.estimate_covariances(X, radius, max_nn, 1e-3, details=True)
    with np.errstate(invalid="ignore"):
        well = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-6
    return X, radius, ref, lam, np.nonzero(~well & ~np.isnan(lam[:, 0]))[0]


def gicp_small():
    out = icp_step_small("ggi")
    for max_nn in (8, 100):  # both list capacities of the covariance kernel
        X, radius, ref, lam, skip = covariance_reference(max_nn)
        got = tp.estimate_covariances(X, radius, max_nn, 1e-3)
        gi.check_covariances(got, ref, lam, skip)
        out.append(got)
    return out


def gicp_large():
    icp_step_large("ggi_768_gap")
    P, Q, _, _ = RI0.config5_problem()
    tp.estimate_covariances_batch([P, Q], 0.1, 100, 1e-3)  # sizes the buffers; its comparison is tests/test_gpu_icp_gicp.py's


@fills
def test_generalized_icp_and_covariance_estimation(fill):
    independent("gicp", fill, fill_of("icp"), gicp_large, gicp_small)


# ---- Colored ICP ------------------------------------------------------------------------------------------------------
COLORED = (0, 1, 2)  # scenes of icp_colored_reference.wide_batch(): the Huber, Cauchy and Tukey kernels in turn


@memo
def colored_cases():
    w = RC.wide_batch()
    out = []
    for i in COLORED:
        s = w[i]
        g = RC.color_gradients(s["target"], s["target_normals"], s["target_colors"], 2 * s["r"], 30)
        reg = RC.registration_icp(s["source"], s["target"], s["source_colors"], s["target_colors"], s["target_normals"],
                                  s["r"], kernel=s["kernel"][0], k=s["kernel"][1], gradients=g,
                                  max_iteration=RC.WIDE_ITERATIONS, margins=True)
        out.append((s, g, reg))
    assert all(r["margins"]["best_gap"] > 1e-7 and r["margins"]["radius_gap"] > 1e-7 and r["margins"]["stop_gap"] > 1e-9
               for _, _, r in out)  # equal decisions are a fair demand (tests/wide_batch_cases.py)
    return out


def check_colored(g, r, what):
    """The comparison of tests/test_gpu_icp_colored.py and tests/test_gpu_wide_batches.py, with their bars."""
    assert g.iterations == r["iterations"], what
    assert np.array_equal(g.correspondence_set, r["correspondence_set"]), what
    assert np.linalg.norm(g.transformation - r["transformation"]) < 1e-9, what
    assert abs(g.fitness - r["fitness"]) <= 1e-12 * max(r["fitness"], 1e-300), what
    assert abs(g.inlier_rmse - r["inlier_rmse"]) <= 1e-12 * max(r["inlier_rmse"], 1e-300), what


def colored_small():
    crit = tp.ICPConvergenceCriteria(max_iteration=RC.WIDE_ITERATIONS)
    out = []
    for i, (s, g, reg) in zip(COLORED, colored_cases()):
        grad = tp.estimate_color_gradients(s["target"], s["target_normals"], s["target_colors"], 2 * s["r"], 30)
        assert grad.shape == g.shape and grad.tobytes() == g.tobytes(), i
        res = col.run_colored(s, col.colored(*s["kernel"]), crit)
        check_colored(res, reg, i)
        out += [grad, icp_fields(res)]
    cases = colored_cases()
    batch = tp.registration_icp_batch([s["source"] for s, _, _ in cases], [s["target"] for s, _, _ in cases], RC.WIDE_R,
                                      criteria=crit, estimation_methods=[col.colored(*s["kernel"]) for s, _, _ in cases],
                                      target_normals=[s["target_normals"] for s, _, _ in cases],
                                      source_colors=[s["source_colors"] for s, _, _ in cases],
                                      target_colors=[s["target_colors"] for s, _, _ in cases])
    for i, (res, (_, _, reg)) in enumerate(zip(batch, cases)):
        check_colored(res, reg, ("batch", i))
    return out + [icp_fields(r) for r in batch]


@memo
def colored_scene_reference():
    s = scene()
    return RC.registration_icp(s["source"], s["target"], s["source_colors"], s["target_colors"], s["target_normals"],
                               s["r"], kernel="l2", k=1.0, gradients=scene_gradients(0, 30), max_iteration=2)


def colored_large():
    """The textured scene (2 304 target points): its gradients bit for bit, two iterations by the front-end's comparison."""
    s = scene()
    grad = tp.estimate_color_gradients(s["target"], s["target_normals"], s["target_colors"], 2 * s["r"], 30)
    assert grad.tobytes() == scene_gradients(0, 30).tobytes()
    check_colored(col.run_colored(s, col.colored("l2", 1.0), tp.ICPConvergenceCriteria(max_iteration=2)),
                  colored_scene_reference(), "scene")


@fills
def test_colored_icp(fill):
    independent("colored", fill, fill_of("icp"), colored_large, colored_small)


# ---- information matrices ---------------------------------------------------------------------------------------------
@memo
def information_case(n_s, n_t=300):
    P, Q, Tm = grid_pair(100 + n_s, n_s, n_t)
    return P, Q, Tm, RIN.information(P, Q, 0.5, Tm)


def check_information(info, res, ref, what):
    assert np.array_equal(res.correspondence_set, ref["correspondence_set"]), what
    assert info.tobytes() == (ref["information"] + 0.0).tobytes(), what
    assert res.fitness == ref["fitness"], what


def information_run(sizes):
    cases = [information_case(n) for n in sizes]
    out = []
    for n, (P, Q, Tm, ref) in zip(sizes, cases):
        info, res = tp.get_information_matrix_from_point_clouds_batch([P], [Q], 0.5, Tm, return_results=True)
        check_information(info[0], res[0], ref, n)
        out.append((info[0], icp_fields(res[0])))
    info, res = tp.get_information_matrix_from_point_clouds_batch([c[0] for c in cases], [c[1] for c in cases], 0.5,
                                                                 np.stack([c[2] for c in cases]), return_results=True)
    for n, i, r, c in zip(sizes, info, res, cases):
        check_information(i, r, c[3], ("batch", n))
    return out + [i for i in info]


@fills
def test_information_matrices(fill):
    independent("information", fill, fill_of("icp"), lambda: information_run((2 * 256 + 188,)),
                lambda: information_run((0, 255, 256, 257)))


# ---- self k-NN and both outlier removals ------------------------------------------------------------------------------
@memo
def cloud(n, seed=None):
    return np.random.default_rng(100 + n if seed is None else seed).random((n, 3))


def outlier_run(sizes, ks):
    out = []
    for cap in ring_caps():
        for n in sizes:
            P = cloud(n)
            got = tp.self_knn_batch([P] * len(ks), list(ks), return_distance=True)
            for k, g in zip(ks, got):
                ol.check_knn(P, k, g)
            res = tp.remove_statistical_outlier_batch([P] * len(ks), list(ks), 1.5, return_stats=True)
            for k, g in zip(ks, res):
                ol.check_statistical(P, k, 1.5, g)
            rad = tp.remove_radius_outlier_batch([P, P], [1, 4], [0.2, 0.35], return_counts=True)
            ol.check_radius(P, 1, 0.2, rad[0])
            ol.check_radius(P, 4, 0.35, rad[1])
            out += [got, [(g[0], g[1], g[2]["avg"]) for g in res], rad]
    return out


def outlier_small():
    return outlier_run((255, 256, 257), (1, 33, 100))


def outlier_large():
    return outlier_run((513,), (100,))  # the largest size of tests/test_gpu_outlier.py's block-edge list


@fills
def test_self_knn_and_outlier_removal(fill):
    independent("outlier", fill, fill_of("icp"), outlier_large, outlier_small)


# ---- normal estimation and the point-to-plane entry that estimates its own normals -------------------------------------
@memo
def normals_reference_of(n, sp_key):
    return nm.reference(RN.cube(n, seed=n), normal_search(sp_key))


def normal_search(key):
    return nm.KNN(key[1]) if key[0] == "knn" else nm.Hybrid(key[1], key[2])


NORMAL_SEARCHES = (("knn", 33), ("knn", 100), ("hybrid", 0.17, 33))


def normals_run(sizes):
    out = []
    for cap in ring_caps():
        for key in NORMAL_SEARCHES:
            sp = normal_search(key)
            clouds = [RN.cube(n, seed=n) for n in sizes]
            got = nm.run(clouds, sp)
            for n, g in zip(sizes, got):
                nm.check(g, normals_reference_of(n, key), "%s n %d cap %d" % (sp, n, cap))
            out.append(got)
    return out


def auto_icp_small():
    """teaser_hip_icp_batch_auto: the front-end's own comparison (tests/test_gpu_normals.py) is bit equality with the two
    calls it stands for, normal estimation (compared with its restatement above) and point-to-plane ICP on those normals."""
    dst = RN.cube(257, seed=257)
    src = np.ascontiguousarray(dst[:200] + 0.01)
    crit = tp.ICPConvergenceCriteria(max_iteration=5)
    out = []
    for sp in (nm.KNN(10), nm.Hybrid(0.4, 20)):
        auto = tp.registration_icp(src, dst, 0.3, np.eye(4), nm.Plane(), crit, target_normals=sp)
        normals = tp.estimate_normals_batch([dst], sp)[0]
        two = tp.registration_icp(src, dst, 0.3, np.eye(4), nm.Plane(), crit, target_normals=normals)
        assert blob(icp_fields(auto)) == blob(icp_fields(two)), sp
        assert auto.iterations >= 1 and auto.fitness > 0.5
        out.append(icp_fields(auto))
    return out


def normals_small():
    return normals_run((255, 256, 257)) + auto_icp_small()


def normals_large():
    return normals_run((513,))


@fills
def test_normal_estimation_and_self_estimating_point_to_plane(fill):
    independent("normals", fill, fill_of("icp"), normals_large, normals_small)


# ---- ISS keypoints ----------------------------------------------------------------------------------------------------
ISS_SMALL = [(RN.cube(n, n), p) for n in (63, 64, 65) for p in (dict(), dict(salient_radius=0.4, non_max_radius=0.3))] + \
    [(RN.cube(257, 7), dict(salient_radius=0.3, min_neighbors=3, gamma_21=0.9, gamma_32=0.8))]
ISS_LARGE = [(RN.cube(600, 21), dict(kp.WIDE)), (RN.cube(600, 21), dict())]


def iss_run(items):
    out = []
    for cap in ring_caps():  # the automatic radii come from a self k-NN stage
        for X, p in items:
            got = kp.run([X], [p])[0]
            kp.check(got, X, p, "n %d cap %d" % (len(X), cap))
            out.append((got[0], got[1]["saliency"], got[1]["count"]))
        got = kp.run([X for X, _ in items], [p for _, p in items])
        for (X, p), g in zip(items, got):
            kp.check(g, X, p, "batch n %d cap %d" % (len(X), cap))
    return out


@fills
def test_iss_keypoints(fill):
    independent("iss", fill, fill_of("icp"), lambda: iss_run(ISS_LARGE), lambda: iss_run(ISS_SMALL))


# ---- DBSCAN -----------------------------------------------------------------------------------------------------------
DBSCAN_SMALL = ("contested", "chain_shuffled", "identical")


@memo
def dbscan_scenes():
    return RD.builders()


@memo
def dbscan_largest():
    return max(dbscan_scenes(), key=lambda name: len(dbscan_scenes()[name][0]))


def dbscan_run(names):
    built = [dbscan_scenes()[n] for n in names]
    out = []
    for n, (P, eps, mp) in zip(names, built):
        got = db.run([P], eps, mp)[0]
        db.check(got, RD.expected(n), n)
        out.append(got)
    got = db.run([b[0] for b in built], [b[1] for b in built], [b[2] for b in built])
    for n, g in zip(names, got):
        db.check(g, RD.expected(n), "batch " + n)
    return out


@fills
def test_dbscan(fill):
    independent("dbscan", fill, fill_of("icp"), lambda: dbscan_run((dbscan_largest(),)), lambda: dbscan_run(DBSCAN_SMALL))


# ---- farthest-point down-sampling, both routes ------------------------------------------------------------------------
@memo
def fps_case(kind, n):
    P = RFP.lattice(np.random.default_rng(n), n) if kind == "lattice" else RFP.gaussian(np.random.default_rng(n), n)
    return P


def fps_run(items):
    out = []
    for kind, n, K in items:
        P = fps_case(kind, n)
        got = fpsm.both_routes([P, P], K, [0, n - 1])  # resident and streamed: the same bytes
        for g, s in zip(got, (0, n - 1)):
            fpsm.check(g, P, K, s, "%s n %d start %d" % (kind, n, s))
        out.append(got)
    return out


def fps_small():
    return fps_run([("lattice", n, 48) for n in (255, 256, 257)] + [("lattice", RFP.WIDE_CAPACITY + 1, 48)])


def fps_large():
    return fps_run([("gaussian", 4097, 64), ("lattice", RFP.WIDE_CAPACITY + 1, 48)])


@fills
def test_farthest_point_down_sampling(fill):
    assert fpsm.capacity() == RFP.WIDE_CAPACITY
    independent("fps", fill, fill_of("icp"), fps_large, fps_small)


# ---- two-cloud search: k-NN, radius, hybrid ---------------------------------------------------------------------------
@memo
def search_pair(nd, nq):
    rng = np.random.default_rng(1000 * nd + nq)
    return rng.random((nd, 3)), rng.random((nq, 3)) * 1.5 - 0.25  # a good part of the queries outside the data's box


@memo
def search_reference(nd, nq, k):
    P, Q = search_pair(nd, nq)
    return RS.knn_search(P, Q, k)


def search_run(pairs, ks):
    out = []
    data, query = [search_pair(*p)[0] for p in pairs], [search_pair(*p)[1] for p in pairs]
    for cap in ring_caps():
        for k in ks:
            got = tp.knn_search_batch(data, query, k)
            for (nd, nq), g in zip(pairs, got):
                se.assert_knn(g, search_reference(nd, nq, k), "n_data %d n_query %d k %d cap %d" % (nd, nq, k, cap))
            one = tp.knn_search(data[0], query[0], k)
            se.assert_knn(one, search_reference(*pairs[0], k), "alone k %d cap %d" % (k, cap))
            out.append(got)
    for P, Q in zip(data, query):
        for max_nn in (1, 33, 100):
            got = tp.hybrid_search(P, Q, 0.2, max_nn)
            se.assert_hybrid(got, P, Q, 0.2, max_nn)
            out.append(got)
        got = tp.radius_search(P, Q, 0.2)
        se.assert_radius(got, P, Q, 0.2)
        out.append(got)
    return out


def search_small():
    return search_run([(255, 64), (256, 65), (257, 130)], (1, 33, 100))


def search_large():
    return search_run([(4097, 130)], (100,))


@fills
def test_two_cloud_search(fill):
    independent("search", fill, fill_of("icp"), search_large, search_small)


# ---- Open3D-form FPFH and boundary points -----------------------------------------------------------------------------
SMALL_LIST_BYTES = 64 * 10 * 12  # the bound both front-ends' own tests set for the second route (the lists in pieces)


def list_front_end(mod, names, all_cases=False):
    """The FPFH or boundary cases `names` (all of the list: the warm-up), each alone and in one batch, at the default
    fpfh_list_bytes and at the small one, at both ring caps."""
    every = [c[0] for c in mod.cases()]
    sel = list(range(len(every))) if all_cases else [every.index(n) for n in names]
    default = tp.get_icp_option("fpfh_list_bytes")
    out = []
    try:
        for bound in (default, SMALL_LIST_BYTES):
            tp.set_icp_option("fpfh_list_bytes", bound)
            for cap in ring_caps():
                if not all_cases:
                    for k in sel:
                        got = mod.run([k])
                        mod.check([k], got, "alone, bound %d cap %d" % (bound, cap))
                        out.append(got)
                got = mod.run(sel)
                mod.check(sel, got, "one batch, bound %d cap %d" % (bound, cap))
    finally:
        tp.set_icp_option("fpfh_list_bytes", default)
    return out


FPFH_SMALL = ("n63", "n64", "n65", "n257", "knn_100")
BOUNDARY_SMALL = ("n63", "n64", "n65", "n257", "knn33", "knn65")


@fills
def test_fpfh_open3d_form(fill):
    independent("fpfh", fill, fill_of("icp"), lambda: list_front_end(fp, (), True), lambda: list_front_end(fp, FPFH_SMALL))


@fills
def test_boundary_points(fill):
    independent("boundary", fill, fill_of("icp"), lambda: list_front_end(bd, (), True),
                lambda: list_front_end(bd, BOUNDARY_SMALL))


# ---- depth frames: unprojection and projection ------------------------------------------------------------------------
UNPROJECT_SMALL = ("7x5_stride1", "7x5_stride2", "color1_intensity0_padded", "color3_intensity0_padded", "257x1")
PROJECT_SMALL = ("one", "3x2", "duplicates", "crowd_1x1")


def unproject_run(names):
    sel = [rg.uindex(n) for n in names]
    out = []
    for k in sel:
        got = rg.unproject([k])
        rg.check_unprojection([k], got, "alone")
        out.append([(r.points, r.colors, r.pixels) for r in got])
    got = rg.unproject(sel)
    rg.check_unprojection(sel, got, "one batch")
    return out


def unproject_large():
    everything = list(range(len(rg.ucases())))
    rg.check_unprojection(everything, rg.unproject(everything), "the list")


def project_run(names):
    sel = [rg.pindex(n) for n in names]
    out = []
    for k in sel:
        got = rg.project([k])
        rg.check_projection([k], got, "alone")
        out.append([(r.depth, r.color, r.index, r.n_hit) for r in got])
    got = rg.project(sel)
    rg.check_projection(sel, got, "one batch")
    return out


def project_large():
    everything = list(range(len(rg.pcases())))
    rg.check_projection(everything, rg.project(everything), "the list")


@fills
def test_unprojection(fill):
    independent("unproject", fill, fill_of("icp"), unproject_large, lambda: unproject_run(UNPROJECT_SMALL))


@fills
def test_projection(fill):
    independent("project", fill, fill_of("icp"), project_large, lambda: project_run(PROJECT_SMALL))


# ---- RGB-D odometry and its pyramid stage -----------------------------------------------------------------------------
ODOMETRY_SMALL = ("8x8", "37x29", "block+1", "singular", "no_correspondence")
ODOMETRY_MIXED = ["37x29", "8x8", "no_correspondence", "singular_3_levels", "f32_specials", "4x4"]  # options (3, 2, 2)


def odometry_fields(r):
    t = r.trace
    return (r.success, r.count, r.iterations, r.transformation, r.information, t.level, t.executed, t.count, t.failed,
            t.e, t.A, t.g, t.pose)


def pyramid_run(name):
    cs = ROD.cases()[name]
    src, tgt = od.images(cs.pair)
    levels = tp.rgbd_odometry_pyramid_batch([src], [tgt], od.intrinsic(cs.pair), cs.pair.odo_init, od.option(cs.opt))[0]
    ref = ROD.result(name).levels
    assert len(levels) == len(ref)
    for l, (got, want) in enumerate(zip(levels, ref)):
        for plane in ("I_s", "I_t", "D_s", "D_t", "I_t_dx", "I_t_dy", "D_t_dx", "D_t_dy"):
            assert np.array_equal(od.bits(got[plane]), od.bits(want[plane])), (name, l, plane)
        assert od.same(got["XYZ"], np.stack([want["X"], want["Y"], want["Z"]], axis=2)), (name, l, "XYZ")
    return levels


def odometry_run(names, mixed=None):
    out = []
    for n in names:
        got = od.run([n])[0]
        od.check_result(got, n)
        out.append(odometry_fields(got))
    if mixed:
        assert len({ROD.cases()[n].opt.iterations for n in mixed}) == 1
        for got, n in zip(od.run(mixed), mixed):
            od.check_result(got, n)
            out.append(odometry_fields(got))
    return out


def odometry_small():
    return odometry_run(ODOMETRY_SMALL, ODOMETRY_MIXED) + [pyramid_run("8x8"), pyramid_run("37x29")]


def odometry_large():
    return odometry_run(("group+1",)) + [pyramid_run("group+1")]


@fills
def test_rgbd_odometry(fill):
    assert not ROD.result("singular").success and ROD.result("no_correspondence").count == 0
    independent("odometry", fill, fill_of("icp"), odometry_large, odometry_small)


# ---- voxel down-sampling ----------------------------------------------------------------------------------------------
@memo
def voxel_case(name):
    rng = np.random.default_rng(77)
    if name == "scan":
        P, v = RV.scan_like(), 0.05
    elif name == "wide_grid":  # more than 2^21 voxels per axis: the two-word keys and the second sort pass
        P, v = rng.uniform(0, 5e6, size=(2000, 3)), 1.0
        assert (RV.voxel_indices(P, v).max(0) >= 2 ** 21).all()
    else:
        P, v = cloud(int(name)), 0.05
    return P, v, RV.voxel_down_sample(P, v)


def voxel_run(names):
    out = []
    for n in names:
        P, v, ref = voxel_case(n)
        got = vx.gpu(P, v)
        vx.assert_bits(got, ref)
        out.append(got)
    return out


@fills
def test_voxel_down_sampling(fill):
    independent("voxel", fill, fill_of("voxel"), lambda: voxel_run(("scan", "wide_grid")),
                lambda: voxel_run(("1", "255", "257", "wide_grid", "scan")))


# ---- the features handle: FPFH, the 1-NN and k-NN matchers, the tuple test --------------------------------------------
@memo
def fpfh_cases():
    C5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    vox = float(C5["voxel_size"])
    cases = [(fb.G["matcher_object"], 0.02, 0.04), (fb.sparse_cloud(), 0.03, 0.05), (C5["cloud_bin_0"], 2 * vox, 5 * vox)]
    cases.sort(key=lambda c: len(c[0]))
    return [(p, rn, rf) + tuple(F.fpfh_features(p, rn, rf)) for p, rn, rf in cases]


def features_fpfh_run(sel):
    cases = [fpfh_cases()[k] for k in sel]
    out = []
    for pts, rn, rf, fo, no in cases:
        f, nrm = tp.compute_fpfh_batch([pts], rn, rf, return_normals=True)
        assert fb.same(nrm[0], no) and fb.same(f[0], fo), len(pts)
        out.append((f[0], nrm[0]))
    f, nrm = tp.compute_fpfh_batch([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], return_normals=True)
    for k, c in enumerate(cases):
        assert fb.same(nrm[k], c[4]) and fb.same(f[k], c[3]), ("batch", k)
    return out


@fills
def test_features_fpfh(fill):
    independent("features_fpfh", fill, fill_of("features"), lambda: features_fpfh_run((2,)),
                lambda: features_fpfh_run((0, 1, 2)))


@memo
def matcher_cases():
    """Of tests/test_gpu_features_batch.py's edge pairs: 255 / 256 / 257 rows against 64 / 65 / 130, both orders, the
    tie pair, and the largest (513 against 130), with the oracle's matches."""
    src, dst = fb.edge_features(33)
    want = [(255, 64), (256, 65), (257, 130), (513, 130)]
    sel = [2 * fb.EDGE_N.index(p) + o for p in want for o in (0, 1)] + [len(src) - 2, len(src) - 1]
    return [(src[k], dst[k], {c: F.match(src[k], dst[k], crosscheck=c) for c in (True, False)}) for k in sel]


def matcher_run(sel):
    cases = [matcher_cases()[k] for k in sel]
    out = []
    for cross in (True, False):
        got = tp.match_features_batch([c[0] for c in cases], [c[1] for c in cases], use_crosscheck=cross)
        for k, (g, c) in enumerate(zip(got, cases)):
            assert fb.same(g, c[2][cross]), (cross, k)
        one = tp.match_features_batch([cases[0][0]], [cases[0][1]], use_crosscheck=cross)[0]
        assert fb.same(one, cases[0][2][cross]), cross
        out.append(got)
    return out


@fills
def test_features_matcher_1nn(fill):
    independent("features_match", fill, fill_of("features"), lambda: matcher_run(range(len(matcher_cases()))),
                lambda: matcher_run((0, 1, 2, 3, 4, 5, 8, 9)))


def knn_matcher_run(nds, ks):
    data, query, ref = fk.edge_problems(33)
    sel = [len(fk.NQ) * fk.ND.index(nd) + q for nd in nds for q in range(len(fk.NQ))]
    out = []
    for k in ks:
        idx, dist = tp.knn_features_batch([data[p] for p in sel], [query[p] for p in sel], k, return_distance=True)
        for p, i, d in zip(sel, idx, dist):
            ri, rd = ref[p]
            assert fk.same(i, np.ascontiguousarray(ri[:, :k])) and fk.same(d, np.ascontiguousarray(rd[:, :k])), (k, p)
        out.append((idx, dist))
    src, dst = fk.mixed_batch()
    for k, mutual in ((3, True), (16, False)):
        batch = tp.match_features_knn_batch(src, dst, k, mutual)
        for p in range(len(src)):
            assert fk.same(batch[p], knn_match_reference(p, k, mutual)), (k, mutual, p)
        out.append(batch)
    return out


@memo
def knn_match_reference(p, k, mutual):
    src, dst = fk.mixed_batch()
    return fk.R.match_knn(src[p], dst[p], k, mutual)


@fills
def test_features_matcher_knn(fill):
    independent("features_knn", fill, fill_of("features"), lambda: knn_matcher_run((513,), (16,)),
                lambda: knn_matcher_run((255, 256, 257), (1, 5, 16)))


@memo
def tuple_cases():
    src, dst, pairs = RT.scene()
    parts = [pairs[:n] for n in (63, 64, 65, 257)] + [pairs[-257:], pairs]
    return src, dst, parts, [tt.host(src, dst, part, RT.SCALE, 11) for part in parts]


@memo
def tuple_large():
    cl, _, pairs = RT.large_problem()
    return cl, pairs, tt.host(cl, cl, pairs, 0.9, 3)


def tuple_run(large):
    src, dst, parts, want = tuple_cases()
    out = []
    for part, w in zip(parts, want):
        got = tp.tuple_test_batch([src], [dst], [part], RT.SCALE, 11)[0]
        assert tt.same(got, w), len(part)
        out.append(got)
    got = tp.tuple_test_batch([src] * len(parts), [dst] * len(parts), parts, RT.SCALE, 11)
    assert all(tt.same(g, w) for g, w in zip(got, want))
    if large:
        cl, pairs, w = tuple_large()
        got = tp.tuple_test_batch([cl, src], [cl, dst], [pairs, parts[-1]], [0.9, RT.SCALE], [3, 11])
        assert tt.same(got[0], w) and tt.same(got[1], want[-1])
        out.append(got[0])
    return out


@fills
def test_features_tuple_test(fill):
    independent("features_tuple", fill, fill_of("features"), lambda: tuple_run(True), lambda: tuple_run(True))


# ---- pose graphs ------------------------------------------------------------------------------------------------------
POSEGRAPH_SMALL = ("trivial_no_edge", "n2_m1", "consistent", "gross_chord")
POSEGRAPH_LARGE = "size_128"


def posegraph_optimize(names):
    built = [pg.objects(PC.build(n)[2]) for n in names]
    out = []
    for n, (crit, option) in zip(names, built):
        res = tp.global_optimization_batch([pg.pose_graph(n)], tp.GlobalOptimizationLevenbergMarquardt(), crit, option,
                                           trace=pg.TRACE)[0]
        PC.check_against_reference(n, pg.as_got(res), report=lambda line: None)
        out.append(pg.bits(res))
    batch = tp.global_optimization_batch([pg.pose_graph(n) for n in names], tp.GlobalOptimizationLevenbergMarquardt(),
                                         [b[0] for b in built], [b[1] for b in built], trace=pg.TRACE)
    for n, res, one in zip(names, batch, out):
        assert pg.bits(res) == one, n
    return out


@memo
def linearize_reference(name):
    start, edges, opt = PC.build(name)
    return PGR.linearize(start, edges, opt, np.float64), PGR.linearize(start, edges, opt, np.longdouble)


def posegraph_linearize(names):
    """The comparison of tests/test_gpu_posegraph.py's linearize test: at most 16 times the restatement's own noise."""
    out = []
    for n in names:
        got = tp.linearize_pose_graph(pg.pose_graph(n), pg.objects(PC.build(n)[2])[1])
        l64, lld = linearize_reference(n)
        ratios = {k: PC.ratio(got[k], l64[k], lld[k]) for k in ("e", "r", "l", "mu", "F", "H", "g")}
        assert max(ratios.values()) <= 16.0, (n, ratios)
        assert np.array_equal(got["H"], got["H"].T)
        out.append([got[k] for k in ("e", "r", "l", "mu", "F", "H", "g")])
    return out


def posegraph_run(names, linear):
    return posegraph_optimize(names) + posegraph_linearize(linear)


@fills
def test_pose_graph_optimisation(fill):
    assert PC.WIDE
    independent("posegraph", fill, fill_of("posegraph"), lambda: posegraph_run((POSEGRAPH_LARGE,), (POSEGRAPH_LARGE,)),
                lambda: posegraph_run(POSEGRAPH_SMALL + (POSEGRAPH_LARGE,), ("n2_m1", "consistent")))


# ---- RANSAC on correspondences ----------------------------------------------------------------------------------------
RANSAC_BY_SIZE = sorted(rs.CASES, key=lambda n: len(rs.G[n + "/corr"]))
RANSAC_SMALL, RANSAC_LARGE = tuple(RANSAC_BY_SIZE[:2]), RANSAC_BY_SIZE[-1]


def ransac_trials(name, n):
    c = rs.case(name)
    return tp.ransac_trials_batch([c["P"]], [c["Q"]], [c["corr"]], c["r"], 0, n, None, c["ransac_n"], rs.checkers_of(c),
                                  c["seed"])[0]


def ransac_stage(name, n):
    """The per-trial records against the restatement evaluated on the device's transformations, bit for bit (the
    comparison of tests/test_gpu_ransac.py, stages 1 and 3)."""
    dev = ransac_trials(name, n)
    ref = rs.restated(name, 0, n, True, dev["transformation"])
    for k in ("samples", "flags", "count"):
        assert np.array_equal(dev[k], ref[k]), (name, k)
    assert np.array_equal(rs.bits(dev["sum_d2"]), rs.bits(ref["sum_d2"])), name
    return dev


def ransac_full(name):
    """The full call against the restatement's loop over the device's own records (stage 4 of tests/test_gpu_ransac.py)."""
    c = rs.case(name)
    max_iteration, confidence = int(rs.G[name + "/criteria"][0]), float(rs.G[name + "/criteria"][1])
    dev = ransac_trials(name, max_iteration)
    want = RR.loop(lambda first, n: {k: v[first:first + n] for k, v in dev.items()}, len(c["corr"]), c["ransac_n"],
                   max_iteration, confidence)
    got = rs.full_call(name)
    assert (got.best_trial, got.trials, got.valid_trials) == (want["best_trial"], want["trials"], want["valid_trials"])
    assert rs.bits(got.fitness) == rs.bits(want["fitness"]) and rs.bits(got.inlier_rmse) == rs.bits(want["inlier_rmse"])
    assert np.array_equal(rs.bits(got.transformation), rs.bits(dev["transformation"][got.best_trial]))
    assert len(got.correspondence_set) == want["count"]
    return rs.result_bits(got)


def ransac_run(names):
    out = [blob(ransac_stage(n, 257)) for n in names]
    out += [ransac_full("early"), ransac_full("full")]
    P, Q, corr, kw = rs.mixed_batch()
    out.append([rs.result_bits(r) for r in tp.registration_ransac_based_on_correspondence_batch(P, Q, corr, **kw)])
    return out


@fills
def test_ransac_on_correspondences(fill):
    independent("ransac", fill, fill_of("ransac"), lambda: ransac_stage(RANSAC_LARGE, rs.TRIALS),
                lambda: ransac_run(RANSAC_SMALL + (RANSAC_LARGE,)))


# ---- FGR on correspondences -------------------------------------------------------------------------------------------
FGR_SMALL, FGR_LARGE = ("c9", "c10", "c63"), "c1025"


def check_fgr(name, r):
    """The comparison of tests/test_gpu_fgr.py's end-to-end test, with its bar (16 times the float64 restatement's
    distance to the longdouble one)."""
    d = float(np.abs(r.transformation.astype(fg.LD) - fg.gold(name, "transformation")).max())
    counts = fg.G[name + "/counts"]
    assert (r.fgr["iterations"], r.fgr["failed_solves"], r.fgr["flags"]) == tuple(int(v) for v in counts), name
    assert abs(r.fgr["final_mu"] - float(fg.G[name + "/final_mu_hi"])) <= 16 * fg.EPS * r.fgr["final_mu"], name
    assert d <= 16 * float(fg.G[name + "/distance_f64"]), name


def fgr_run(names):
    out = []
    for n in names:
        r = fg.full([n])[0]
        check_fgr(n, r)
        out.append(fg.raw(r))
    for knob in (256, 0):  # every problem resident, every problem streamed: the same bits
        for n, r, one in zip(names, fg.full(list(names), knob), out):
            check_fgr(n, r)
            assert fg.raw(r) == one, (knob, n)
    ins = [fg.inputs(n) for n in names if fg.iterations(n) >= 3]
    opts = [fg.option(n) for n in names if fg.iterations(n) >= 3]
    recs = tp.fgr_iterations_batch([a[0] for a in ins], [a[1] for a in ins], [a[2] for a in ins], 3, opts)
    return out + [blob(r) for r in recs]


@fills
def test_fgr_on_correspondences(fill):
    assert tp.get_fgr_option("resident_max_corr") == 256
    independent("fgr", fill, fill_of("fgr"), lambda: fgr_run((FGR_LARGE,)), lambda: fgr_run(FGR_SMALL + (FGR_LARGE,)))


# ---- plane segmentation -----------------------------------------------------------------------------------------------
PLANE_SMALL, PLANE_LARGE = ("too_few", "no_iterations", "exact_plane", "never_stops"), "stops_early"


@memo
def plane_trials_reference(cnt, ransac_n):
    return PR.trials(pl.CLOUD, pl.D, ransac_n, 100 + ransac_n, 0, cnt)


def plane_run(names):
    out = []
    for n in names:
        dev = pl.run(n)
        pl.same_result(dev, pl.restated(n))
        out.append(dev)
    cs = [pl.FULL[n] for n in names]
    batch = tp.segment_plane_batch([c["P"] for c in cs], [c["d"] for c in cs], [c["ransac_n"] for c in cs],
                                   [c["num_iterations"] for c in cs], [c["probability"] for c in cs],
                                   [c["seed"] for c in cs])
    for n, dev in zip(names, batch):
        pl.same_result(dev, pl.restated(n))
    for cnt, ransac_n in ((257, 3), (65, 8)):
        dev = tp.plane_trials_batch([pl.CLOUD], pl.D, 0, cnt, ransac_n, 100 + ransac_n)[0]
        pl.same_trials(dev, plane_trials_reference(cnt, ransac_n))
        out.append(dev)
    return out


@fills
def test_plane_segmentation(fill):
    independent("plane", fill, fill_of("plane"), lambda: plane_run((PLANE_LARGE,)),
                lambda: plane_run(PLANE_SMALL + (PLANE_LARGE,)))


# ---- the TSDF volume: integration, both point clouds, the mesh, the ray cast --------------------------------------------
@memo
def tsdf_views(name):
    vol = T.result(name).vol
    thr = 3.0 if name == "sphere" else 1.0
    views = [TR.view(33, 17, np.eye(4), weight_threshold=thr),
             TR.view(17, 9, T.extrinsic(0.05, -0.1, 0.3, (0.02, -0.01, 0.1)), weight_threshold=thr)]
    return views, [TR.cast(vol, w) for w in views]


def tsdf_everything(vol, name):
    cs = T.cases()[name]
    ts.integrate_all(vol, cs.frames)
    ts.check(vol, name)  # the volume, the surface points and the voxel cloud
    tmesh.check(vol, TM.result(name), name)
    views, refs = tsdf_views(name)
    cast = tray.cast(vol, views)
    for k, (g, r) in enumerate(zip(cast, refs)):
        tray.equal(g, r, (name, k))
    mesh = vol.extract_triangle_mesh(vertex_normals=True)
    return (vol.extract_volume_tsdf(), vol.extract_volume_color(), mesh.vertices, mesh.triangles,
            [(g.depth, g.vertex_map, g.normal_map, g.color, g.hits) for g in cast])


@fills
@pytest.mark.parametrize("name", ["r5_rgb", "r16_gray_small", "sphere"])
def test_tsdf_volume(name, fill):
    """A volume is a handle of its own, so there is no larger case to warm with: the calls themselves size its buffers.
    The volume downloaded before and after a fill is the same bytes: the fill spares what is state."""
    cs = T.cases()[name]
    with ts.make_volume(cs) as vol:
        assert vol.fill_scratch(fill) == 0  # a handle that has served no call owns no scratch
        with pytest.raises(tp.TeaserHipError, match="byte must lie in 0..255"):
            vol.fill_scratch(256)
        tsdf_everything(vol, name)
        before = (vol.extract_volume_tsdf(), vol.extract_volume_color())
        filled = vol.fill_scratch(fill)
        assert filled > 0
        after = (vol.extract_volume_tsdf(), vol.extract_volume_color())
        assert blob(before) == blob(after) and before[0].any()
        vol.reset()
        assert vol.fill_scratch(fill) == filled
        got = blob(tsdf_everything(vol, name))
        assert vol.fill_scratch(fill) == filled, "a buffer grew during the calls"
    seen = _seen.setdefault("tsdf_" + name, {})
    seen[fill] = got
    assert all(b == got for b in seen.values())


# ---- cross-front-end order on the ICP handle (no fill) -----------------------------------------------------------------
FRONT_ENDS = {
    "normals": (normals_large, normals_small),
    "colored": (colored_large, colored_small),
    "iss": (lambda: iss_run(ISS_LARGE), lambda: iss_run(ISS_SMALL)),
    "dbscan": (lambda: dbscan_run((dbscan_largest(),)), lambda: dbscan_run(DBSCAN_SMALL)),
    "fpfh": (lambda: list_front_end(fp, (), True), lambda: list_front_end(fp, FPFH_SMALL)),
    "boundary": (lambda: list_front_end(bd, (), True), lambda: list_front_end(bd, BOUNDARY_SMALL)),
    "unproject": (unproject_large, lambda: unproject_run(UNPROJECT_SMALL)),
    "project": (project_large, lambda: project_run(PROJECT_SMALL)),
    "odometry": (odometry_large, odometry_small),
    "point_to_plane": (lambda: icp_step_large("gpl_65793"), lambda: icp_step_small("gpl")),
    "outlier": (outlier_large, outlier_small),
    "search": (search_large, search_small),
}
PAIRS = [("normals", "colored"), ("iss", "dbscan"), ("fpfh", "boundary"), ("unproject", "project"), ("project", "odometry"),
         ("odometry", "point_to_plane"), ("outlier", "search")]


@pytest.mark.parametrize("a,b", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_front_ends_that_share_a_buffer_in_every_order(a, b):
    """A large, B small, A small, B large on the one cached handle; every call compares its results with the restatement."""
    (a_large, a_small), (b_large, b_small) = FRONT_ENDS[a], FRONT_ENDS[b]
    a_large()
    b_small()
    a_small()
    b_large()
