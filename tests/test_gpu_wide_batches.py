"""The front-ends merged after tests/test_gpu_batch_width.py on the MI355X with 320 problems in one call.  Every problem
is compared with the front-end's numpy restatement by the comparison the front-end's own GPU tests use (imported from
them; this file has no tolerance of its own), and problems 0, 63, 64, 65, 255, 256, 257 and 319 with the same problem
called alone, byte for byte.  A wrong blockIdx.x * 256 term, block-map offset or per-problem stride in a kernel that
gives a thread, a lane of a tile or a workgroup to a problem shows only from problem 64 or 256 on; every other test of
these front-ends calls them with at most 16 problems.

The batches come from the reference modules' wide_batch() builders, which assert what each test rests on from the sizes
alone; tests/wide_batch_cases.py computes each restatement once, and tests/test_wide_batch_cases.py runs both without
a GPU.  Each test asserts its regime (more than 256 problems, blocks or tiles; group counts; empty runs) before the
device is called."""
import importlib

import numpy as np
import pytest

import fgr_reference as RF
import fps_reference as RP
import fpfh_o3d_reference as RH
import icp_colored_reference as RC
import information_reference as RI
import odometry_reference as ROD
import plane_reference as PR
import posegraph_cases as PC
import outlier_reference as RO
import ransac_reference as RR
import rgbd_reference as RG
import wide_batch_cases as W
from test_gpu_batch_width import icp_problems
from test_gpu_boundary import param as search_param
from test_gpu_dbscan import check as check_dbscan, run as run_dbscan
from test_gpu_fgr import EPS, LD, raw as fgr_raw
from test_gpu_fps import both_routes as fps_both_routes, capacity as fps_capacity, run as run_fps, same_bytes as same_fps
from test_gpu_icp_colored import colored as colored_estimation, same_bits as same_icp_bits
from test_gpu_information import info_batch
from test_gpu_odometry import (bits as odo_bits, check_result as check_odometry, images as odo_images,
                               intrinsic as odo_intrinsic, jacobian as odo_jacobian, option as odo_option, same as odo_same)
from test_gpu_plane import same_result as same_plane, same_trials as same_plane_trials
from test_gpu_posegraph import TRACE, alone as posegraph_alone, as_got, bits as posegraph_bits, objects, pose_graph
from test_gpu_rgbd import check_projection, check_unprojection, project, unproject
from test_gpu_search import assert_knn
from test_gpu_ransac import bits, result_bits as ransac_bits

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")

B = 320
EDGE = W.EDGE_OF(B)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def blob(x):
    """Every number of a result as bytes, in a fixed order."""
    if isinstance(x, dict):
        return [(k, blob(x[k])) for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [blob(v) for v in x]
    if hasattr(x, "__dict__"):
        return blob(vars(x))
    return np.asarray(x).tobytes()


# ---- plane segmentation ---------------------------------------------------------------------------------------------
def test_plane_segmentation():
    """plane_winner_kernel and plane_fin_total_kernel<0/1> (one lane of a 64-wide tile per problem) in tiles 1 .. 4;
    the model, score, group and total kernels at blockIdx.y / blockIdx.z up to 319; the host plan plan[g * batch + b]
    with two chunks of 64 trials, the second a partial one.  Restatement: 0.3 s on the CPU (stage and full call)."""
    w, ref_trials, ref_full = W.plane()
    clouds, d, rn, its, prob, seed = (w[k] for k in W.PLANE_KEYS)
    assert len(clouds) == B > 256 and min(its) == max(its) > PR.WIDE_CHUNK
    found = [r["best_trial"] >= 0 for r in ref_full]
    assert any(found) and not all(found) and {r["trials"] for r in ref_full} > {0, its[0]}  # some stop early
    before = tp.get_plane_option("chunk_trials")
    try:
        tp.set_plane_option("chunk_trials", PR.WIDE_CHUNK)
        trials = tp.plane_trials_batch(clouds, d, 0, its[0], rn, seed)
        for i in range(B):
            same_plane_trials(trials[i], ref_trials[i])
        got = tp.segment_plane_batch(clouds, d, rn, its, prob, seed)
        for i in range(B):
            same_plane(got[i], ref_full[i])
        for i in EDGE:
            alone = tp.segment_plane_batch([clouds[i]], d[i], rn[i], its[i], prob[i], seed[i])[0]
            assert blob(alone) == blob(got[i]), i
            alone = tp.plane_trials_batch([clouds[i]], d[i], 0, its[i], rn[i], seed[i])[0]
            assert blob(alone) == blob(trials[i]), i
    finally:
        tp.set_plane_option("chunk_trials", before)


# ---- RANSAC on correspondences --------------------------------------------------------------------------------------
def test_ransac_on_correspondences_with_one_to_four_chunks_in_a_group():
    """ransac_chunk_kernel and ransac_prefix_kernel at blockIdx.y up to 319; the Layout, the carried RsBest[batch] and
    the speculative chunks with 1, 2, 3 and 4 chunks in a group (chunk_trials 4096, 3072, 2048, 1024 at 320 problems;
    every other GPU test runs with 4).  Four problems never stop early (5 000, 7 000 and 13 000 trials), twenty stop
    after hundreds of trials, the others after tens, so the open problems thin out group by group.

    The transformation of a trial comes from the device's SVD, which is not numpy's bit for bit (test_gpu_ransac.py
    compares it with a 50-digit pose), so RR.ransac, which estimates with numpy's SVD, cannot be met bit for bit: among
    trials with the same inlier count the smaller rmse wins, and trials that draw the same pairs in another order differ
    in rmse by their last bits only (measured: problem 0, 5 000 trials, best trial 3883 on the device's estimates, 2491
    on numpy's, same count).  So, as in test_gpu_ransac.py: the restatement's per-trial records are evaluated on the
    DEVICE's transformations and compared bit for bit (one stage call over all 320 problems, a second one over the 24
    that run past it), the full call equals the restatement's loop over those records in every bit, and count, rmse
    and inliers of every result equal the restatement's score of the result's own transformation.  With RR.ransac the
    results share the numbers of trials and of valid trials and the inlier count.  Restatement: 5.1 to 6.2 s
    (RR.ransac) on the CPU; the records and loops over the device's transformations are timed with the test only."""
    w, ref = W.ransac()
    assert len(w["P"]) == B > 256
    assert [RR.group_chunks(c, B) for c in RR.WIDE_CHUNKS] == [1, 2, 3, 4]
    done = sorted(r["trials"] for r in ref)
    assert done[-1] == 13000 and done[-4] == 5000 and sum(64 < t < 4096 for t in done) >= 10 and done[2] > 0
    P, Q, corr = w["P"], w["Q"], w["corr"]

    def checkers(i):
        return [tp.CorrespondenceCheckerBasedOnEdgeLength(w["s"][i])] if w["s"][i] > 0 else []

    crit = [tp.RANSACConvergenceCriteria(m, c) for m, c in zip(w["max_iteration"], w["confidence"])]
    kw = dict(max_correspondence_distance=w["r"], ransac_n=w["ransac_n"], checkers=[checkers(i) for i in range(B)],
              criteria=crit, seed=w["seed"])
    before = tp.get_ransac_option("chunk_trials")
    runs = {}
    try:
        for chunk in RR.WIDE_CHUNKS:
            tp.set_ransac_option("chunk_trials", chunk)
            runs[chunk] = tp.registration_ransac_based_on_correspondence_batch(P, Q, corr, **kw)
        tp.set_ransac_option("chunk_trials", before)
        got = runs[before]
        for chunk in RR.WIDE_CHUNKS:
            assert [ransac_bits(r) for r in runs[chunk]] == [ransac_bits(r) for r in got], chunk
        n = RR.WIDE_STAGE
        stage = tp.ransac_trials_batch(P, Q, corr, w["r"], 0, n, None, w["ransac_n"], kw["checkers"], w["seed"])
        late = [i for i in range(B) if ref[i]["trials"] > n]  # their loops end past the first stage call's records
        assert 16 < len(late) < 64
        rest = tp.ransac_trials_batch(*[[w[k][i] for i in late] for k in ("P", "Q", "corr", "r")], 0,
                                      max(w["max_iteration"]), None, [w["ransac_n"][i] for i in late],
                                      [checkers(i) for i in late], [w["seed"][i] for i in late])
        for i in EDGE:
            one = dict(kw, max_correspondence_distance=w["r"][i], ransac_n=w["ransac_n"][i], checkers=checkers(i),
                       criteria=crit[i], seed=w["seed"][i])
            alone = tp.registration_ransac_based_on_correspondence(P[i], Q[i], corr[i], **one)
            assert ransac_bits(alone) == ransac_bits(got[i]), i
            alone = tp.ransac_trials_batch([P[i]], [Q[i]], [corr[i]], w["r"][i], 0, n, None, w["ransac_n"][i],
                                           checkers(i), w["seed"][i])[0]
            assert blob(alone) == blob(stage[i]), i
    finally:
        tp.set_ransac_option("chunk_trials", before)
    records = dict(zip(late, rest))
    for i in range(B):
        g, r = got[i], ref[i]
        args = (P[i], Q[i], corr[i], w["r"][i])
        for dev in [stage[i]] + ([records[i]] if i in records else []):
            m = len(dev["flags"])
            want = RR.trial_records(*args, 0, m, w["ransac_n"][i], w["s"][i], 0.0, w["seed"][i], T=dev["transformation"])
            for k in ("samples", "flags", "count"):
                assert np.array_equal(dev[k], want[k]), (i, k)
            assert np.array_equal(bits(dev["sum_d2"]), bits(want["sum_d2"])), i
        if i in records:
            assert blob({k: v[:n] for k, v in dev.items()}) == blob(stage[i]), i
        # the front-end's own comparison: the restatement's loop over the device's records
        lp = RR.loop(lambda first, m: {k: v[first:first + m] for k, v in dev.items()}, len(corr[i]),
                     w["ransac_n"][i], w["max_iteration"][i], w["confidence"][i])
        assert (g.best_trial, g.trials, g.valid_trials) == (lp["best_trial"], lp["trials"], lp["valid_trials"]), i
        assert bits(g.fitness) == bits(lp["fitness"]) and bits(g.inlier_rmse) == bits(lp["inlier_rmse"]), i
        assert len(g.correspondence_set) == lp["count"], i
        assert (g.trials, g.valid_trials, len(g.correspondence_set)) == (r["trials"], r["valid_trials"], r["count"]), i
        if lp["best_trial"] < 0:
            assert np.array_equal(g.transformation, np.eye(4)) and g.fitness == 0 and g.inlier_rmse == 0, i
            continue
        assert np.array_equal(bits(g.transformation), bits(dev["transformation"][g.best_trial])), i
        count, total, inl = RR.score(g.transformation[None], RR.records_of(*args[:3]), w["r"][i])
        assert np.array_equal(g.correspondence_set, corr[i][inl[0]]), i
        assert bits(g.inlier_rmse) == bits(RR.rmse_of(int(count[0]), float(total[0]))), i


# ---- FGR ------------------------------------------------------------------------------------------------------------
def fgr_options(options, least=0):
    return [tp.FastGlobalRegistrationOption(tuple_test=False, **dict(o, iteration_number=max(o["iteration_number"], least)))
            for o in options]


def test_fgr_on_correspondences_by_both_routes():
    """fgr_finish_kernel (one thread per problem) in its second block of 256; fgr_cloud_* at blockIdx.y up to 319;
    fgr_resident_kernel, and fgr_sums_kernel, fgr_step_kernel and fgr_move_kernel, over index lists of open problems
    that shrink as the iteration numbers 0 .. 16 run out, with every problem resident (resident_max_corr 256), every
    problem streamed (0) and about half down each route (40).  The routes give the same bits; the pose is within the
    front-end's own end-to-end bound of the longdouble restatement (16 x the float64 restatement's distance to it),
    for the full call and for the stage call's three iterations.  Restatement: 3.4 s on the CPU (both calls, in float64
    and in longdouble)."""
    problems, options, full, staged = W.fgr()
    assert len(problems) == B > 256
    its = [o["iteration_number"] for o in options]
    assert len(set(its[256:])) > 4 and min(its) == 0 and max(its) >= 16
    n_res = sum(RF.MIN_CORR <= len(p[2]) <= RF.WIDE_SPLIT for p in problems)
    assert n_res > 128 and B - n_res > 128
    P, Q, corr = ([p[k] for p in problems] for k in range(3))
    opts, stage_opts = fgr_options(options), fgr_options(options, RF.WIDE_STAGE)
    before = tp.get_fgr_option("resident_max_corr")
    assert before == 256
    res, rec = {}, {}
    try:
        for knob in (before, 0, RF.WIDE_SPLIT):
            tp.set_fgr_option("resident_max_corr", knob)
            res[knob] = tp.registration_fgr_based_on_correspondence_batch(P, Q, corr, opts)
            rec[knob] = tp.fgr_iterations_batch(P, Q, corr, RF.WIDE_STAGE, stage_opts)
        tp.set_fgr_option("resident_max_corr", before)
        for i in EDGE:
            alone = tp.registration_fgr_based_on_correspondence(P[i], Q[i], corr[i], opts[i])
            assert blob(alone) == blob(res[before][i]), i
            alone = tp.fgr_iterations_batch([P[i]], [Q[i]], [corr[i]], RF.WIDE_STAGE, stage_opts[i])[0]
            assert blob(alone) == blob(rec[before][i]), i
    finally:
        tp.set_fgr_option("resident_max_corr", before)
    for knob in (0, RF.WIDE_SPLIT):
        for i in range(B):
            assert fgr_raw(res[knob][i]) == fgr_raw(res[before][i]), (knob, i)
            assert blob(rec[knob][i]) == blob(rec[before][i]), (knob, i)
    for i in range(B):
        for dev, (ld, dist) in ((res[before][i].fgr, full[i]), (rec[before][i], staged[i])):
            assert (dev["iterations"], dev["failed_solves"], dev["flags"], dev["n_corr"]) == (
                ld["iterations"], ld["failed_solves"], ld["flags"], len(corr[i])), i
            assert abs(dev["final_mu"] - float(ld["final_mu"])) <= 16 * EPS * dev["final_mu"], i
            assert float(np.abs(dev["transformation"].astype(LD) - ld["transformation"]).max()) <= 16 * dist, i
    assert res[before][150].fgr["flags"] == 1 and res[before][150].fgr["iterations"] == 0


# ---- pose graphs ----------------------------------------------------------------------------------------------------
def test_pose_graph_optimisation():
    """The optimiser's kernel (one workgroup per graph) at blockIdx.x up to 319, with per-graph offsets into the packed
    nodes, edges, traces and results of graphs of 3, 4, 6, 7 and 9 nodes in turn and 128 nodes at 256; the 3-node ring
    has no uncertain edge (Levenberg-Marquardt without a line process), the others have.  Restatement: 1.3 to 1.8 s on
    the CPU (nearly all of it the 128-node graph), in float64 and longdouble."""
    assert PC.WIDE
    names, refs = W.posegraph()
    assert len(names) == B > 256 and names[PC.WIDE_LARGE] == "size_128"
    small = sorted(set(names) - {"size_128"})
    reasons = {refs[n][0]["status"] for n in small}
    built = [objects(PC.build(n)[2]) for n in names]
    out = tp.global_optimization_batch([pose_graph(n) for n in names], tp.GlobalOptimizationLevenbergMarquardt(),
                                       [b[0] for b in built], [b[1] for b in built], trace=TRACE)
    assert len(out) == B
    for i, (name, res) in enumerate(zip(names, out)):
        assert res.n_trace == len(res.trace) <= TRACE, i
        PC.check_against_reference(name, as_got(res), report=lambda line: None)
    assert {res.status for res in out} >= reasons and len(reasons) >= 2  # every stop reason of the small cases
    for i, (name, res) in enumerate(zip(names, out)):  # every graph, not only the edge ones: six graphs alone
        assert posegraph_bits(res) == posegraph_bits(posegraph_alone(name)), (i, name)


# ---- information matrices -------------------------------------------------------------------------------------------
def test_information_matrices():
    """icp_info_block_kernel through a blk_prob of 320 blocks (source sizes 0, 1, 255, 256, 257 in turn) and
    icp_info_finalize_kernel (one workgroup per problem) over each problem's range of block partials, at problems up to
    319; integer grids, so every bit equals numpy's.  Restatement: 2.0 to 3.5 s on the CPU."""
    w, ref = W.information()
    assert len(w) == B > 256
    assert sum((len(p[0]) + RI.K_ICP_BLOCK - 1) // RI.K_ICP_BLOCK for p in w) > 256
    assert not ref[RI.WIDE_FAR]["information"].any() and len(w[RI.WIDE_FAR][0]) >= RI.K_ICP_BLOCK
    assert sum(r["information"].any() for r in ref) > 128
    Ps, Qs, Ts, rs = ([p[k] for p in w] for k in range(4))
    info, res = info_batch(Ps, Qs, rs, np.stack(Ts))
    for i in range(B):
        assert np.array_equal(res[i].correspondence_set, ref[i]["correspondence_set"]), i
        assert info[i].tobytes() == (ref[i]["information"] + 0.0).tobytes(), i
        assert info[i][5, 5] == len(ref[i]["correspondence_set"]), i
        assert res[i].fitness == ref[i]["fitness"], i
    assert not info[RI.WIDE_FAR].any() and len(res[RI.WIDE_FAR].correspondence_set) == 0
    for i in EDGE:
        one, one_res = info_batch([Ps[i]], [Qs[i]], rs[i], Ts[i])
        assert one[0].tobytes() == info[i].tobytes() and blob(one_res[0]) == blob(res[i]), i


# ---- colored ICP ----------------------------------------------------------------------------------------------------
def test_colored_icp_gradients_and_registration():
    """The gradient kernel through a blk_prob of 319 blocks at both list capacities (max_nn 30 for every cloud, then 33,
    64 and 30 in turn), and the iteration kernels' per-problem state at problems up to 319, with the Huber, Cauchy and Tukey
    kernels in turn and three iterations.  Gradients equal the restatement bit for bit; the registration by the
    front-end's own comparison (equal iterations and correspondence sets, ||dT|| < 1e-9, fitness and RMSE within 1e-12
    relative), its decision margins asserted first.  Restatement: 2.3 s + 2.1 s (gradients) + 3.7 s on the CPU."""
    w, g30, gmix, reg = W.colored()
    assert len(w) == B > 256 and sum((len(s["target"]) + 255) // 256 for s in w) > 256
    assert W.colored_margins_hold(reg) and {r["iterations"] for r in reg} >= {1, RC.WIDE_ITERATIONS}
    clouds, normals, colors = ([s[k] for s in w] for k in ("target", "target_normals", "target_colors"))
    radius = [2 * s["r"] for s in w]
    for ref, max_nn in ((g30, [30] * B), (gmix, [W.COLOR_MAX_NN[i % 3] for i in range(B)])):
        got = tp.estimate_color_gradients_batch(clouds, normals, colors, radius, max_nn)
        for i in range(B):
            assert got[i].shape == ref[i].shape and got[i].tobytes() == ref[i].tobytes(), (max_nn[i], i)
        for i in EDGE:
            alone = tp.estimate_color_gradients(clouds[i], normals[i], colors[i], radius[i], max_nn[i])
            assert alone.tobytes() == got[i].tobytes(), i
    crit = tp.ICPConvergenceCriteria(max_iteration=RC.WIDE_ITERATIONS)
    ests = [colored_estimation(*s["kernel"]) for s in w]
    kw = dict(source_colors=[s["source_colors"] for s in w], target_colors=colors)
    got = tp.registration_icp_batch([s["source"] for s in w], clouds, RC.WIDE_R, criteria=crit, estimation_methods=ests,
                                    target_normals=normals, **kw)
    for i, (g, r) in enumerate(zip(got, reg)):
        assert g.iterations == r["iterations"], i
        assert np.array_equal(g.correspondence_set, r["correspondence_set"]), i
        assert np.linalg.norm(g.transformation - r["transformation"]) < 1e-9, i
        assert abs(g.fitness - r["fitness"]) <= 1e-12 * max(r["fitness"], 1e-300), i
        assert abs(g.inlier_rmse - r["inlier_rmse"]) <= 1e-12 * max(r["inlier_rmse"], 1e-300), i
    assert sum(g.fitness > 0.9 for g in got) > 256 and sum(g.fitness == 0 for g in got) == 2
    for i in EDGE:
        s = w[i]
        alone = tp.registration_icp(s["source"], s["target"], s["r"], np.eye(4), ests[i], crit,
                                    source_colors=s["source_colors"], target_colors=s["target_colors"],
                                    target_normals=s["target_normals"])
        assert same_icp_bits(alone, got[i]) and alone.transformation.tobytes() == got[i].transformation.tobytes(), i


# ---- two-cloud search -----------------------------------------------------------------------------------------------
def same_arrays(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_two_cloud_search():
    """k-NN with k = 1, 5, 32, 33, 100 in turn at knn_ring_cap 4 and 0; the hybrid search with the short lists (max_nn
    up to 32) and the long ones (up to 100); the radius search's count, per-problem prefix (dim3(batch)), fill and
    icp_search_rank_kernel, whose binary search over the problems' out_off meets runs of five and more problems
    without an entry (equal offsets), problems 255 .. 257 with entries between such runs, empty data and empty query
    clouds.  Every bit equals the restatement's.  Restatement: 0.1 s on the CPU."""
    w, knn, short, hyb_short, hyb_long, rad = W.search()
    data, query = w["data"], w["query"]
    assert len(data) == B > 256 and sum((len(q) + 255) // 256 for q in query) > 256
    total = [len(r[0]) for r in rad]
    assert sum(total) > 0 and sum(t == 0 for t in total) >= 50
    assert not any(total[250:255]) and all(total[255:258]) and not any(total[258:263])  # the runs around 255 .. 257
    assert any(len(P) == 0 and len(Q) > 0 for P, Q in zip(data, query))
    assert any(len(P) > 0 and len(Q) == 0 for P, Q in zip(data, query))
    before = tp.get_icp_option("knn_ring_cap")
    try:
        for cap in (4, 0):
            tp.set_icp_option("knn_ring_cap", cap)
            got = tp.knn_search_batch(data, query, w["k"])
            for i in range(B):
                assert_knn(got[i], knn[i], "ring cap %d, problem %d" % (cap, i))
            for i in EDGE:
                assert same_arrays(tp.knn_search(data[i], query[i], w["k"][i]), got[i]), (cap, i)
    finally:
        tp.set_icp_option("knn_ring_cap", before)
    for ks, ref in ((short, hyb_short), (w["k"], hyb_long)):
        got = tp.hybrid_search_batch(data, query, w["hybrid_radius"], ks)
        for i in range(B):
            (idx, d2, cnt), (ridx, rd2, rcnt) = got[i], ref[i]
            assert np.array_equal(cnt, rcnt) and np.array_equal(idx, ridx) and RO.bits_equal(d2, rd2), (max(ks), i)
        for i in EDGE:
            assert same_arrays(tp.hybrid_search(data[i], query[i], w["hybrid_radius"][i], ks[i]), got[i]), i
    got = tp.radius_search_batch(data, query, w["radius"])
    for i in range(B):
        (idx, d2, splits), (ridx, rd2, rsplits) = got[i], rad[i]
        assert splits.dtype == np.int64 and np.array_equal(splits, rsplits), i
        assert idx.dtype == np.int32 and np.array_equal(idx, ridx) and RO.bits_equal(d2, rd2), i
    for i in EDGE + (250, 254, 258):
        assert same_arrays(tp.radius_search(data[i], query[i], w["radius"][i]), got[i]), i
    guess = tp.radius_search_batch(data, query, w["radius"], max_total=[max(t - 1, 0) if i % 2 else t + 3 for i, t in enumerate(total)])
    for i in range(B):  # the single-call form, every other problem's guess one entry short
        assert same_arrays(guess[i], got[i]), i


# ---- FPFH (Open3D form) and boundary points -------------------------------------------------------------------------
SMALL_LIST_BYTES = 64 * 10 * 12  # the bound tests/test_gpu_fpfh_o3d.py and test_gpu_boundary.py set for the second route


def two_block_lists(w):
    """The regime of both tests: more than 256 clouds, and more than 128 point blocks in each of the two block lists
    (hybrid, k-NN) that one blk_prob holds one after the other."""
    assert len(w) == B > 256
    for search in (RH.HYBRID, RH.KNN):
        assert sum(1 for c in w if c[2] == search and len(c[0])) > 128


def test_fpfh_open3d_form():
    """The SPFH and FPFH kernels over grids of n_hyb + n_knn point blocks (141 + 139), the two block lists one after
    the other in one blk_prob, at the default fpfh_list_bytes and at the small one that forces the second route (the
    lists computed in pieces).  SPFH and FPFH bits equal the restatement's.  Restatement: 0.6 s on the CPU."""
    w, ref = W.fpfh()
    two_block_lists(w)
    clouds, normals = [c[0] for c in w], [c[1] for c in w]
    params = [search_param(*c[2:]) for c in w]
    default = tp.get_icp_option("fpfh_list_bytes")
    try:
        for bound in (default, SMALL_LIST_BYTES):
            tp.set_icp_option("fpfh_list_bytes", bound)
            got = tp.compute_fpfh_feature_batch(clouds, normals, params, return_spfh=True)
            for i, ((F, H), (Fr, Hr)) in enumerate(zip(got, ref)):
                assert H.shape == Hr.shape and H.tobytes() == Hr.tobytes(), (bound, i)
                assert F.shape == Fr.shape and F.tobytes() == Fr.tobytes(), (bound, i)
            for i in EDGE:
                alone = tp.compute_fpfh_feature_batch([clouds[i]], [normals[i]], [params[i]], return_spfh=True)[0]
                assert blob(alone) == blob(got[i]), (bound, i)
    finally:
        tp.set_icp_option("fpfh_list_bytes", default)
    assert sum(float(F.sum()) > 0 for F, _ in ref) > 128


def test_boundary_points():
    """The boundary kernels over the same two block lists, thresholds of 90, 45 and 170 degrees in turn, at both
    fpfh_list_bytes.  List lengths, largest gaps and masks equal the restatement's.  Restatement: 0.3 s on the CPU."""
    w, ref = W.boundary()
    two_block_lists(w)
    clouds, normals = [c[0] for c in w], [c[1] for c in w]
    params = [search_param(*c[2:]) for c in w]
    angles = [W.BOUNDARY_ANGLES[i % 3] for i in range(B)]
    edge, inner = sum(int(r[0].sum()) for r in ref), sum(int((~r[0].astype(bool)).sum()) for r in ref)
    assert edge > 1000 and inner > 1000
    default = tp.get_icp_option("fpfh_list_bytes")
    try:
        for bound in (default, SMALL_LIST_BYTES):
            tp.set_icp_option("fpfh_list_bytes", bound)
            got = tp.compute_boundary_points_batch(clouds, normals, params, angles, return_max_gap=True,
                                                   return_counts=True)
            for i, (r, (mask, gap, m)) in enumerate(zip(got, ref)):
                assert np.array_equal(r.counts, m), (bound, i)
                assert r.max_gap.tobytes() == gap.tobytes(), (bound, i)
                assert np.array_equal(r.mask, mask) and r.n_boundary == int(mask.sum()), (bound, i)
            for i in EDGE:
                alone = tp.compute_boundary_points_batch([clouds[i]], [normals[i]], [params[i]], [angles[i]],
                                                         return_max_gap=True, return_counts=True)[0]
                assert blob(alone) == blob(got[i]), (bound, i)
    finally:
        tp.set_icp_option("fpfh_list_bytes", default)


# ---- DBSCAN ---------------------------------------------------------------------------------------------------------
def test_dbscan():
    """The four DBSCAN kernels that go through blk_prob, over 280 point blocks of 320 clouds, with eps 0.15, 0.3, 0.6
    and min_points 1, 3, 6 in every pairing.  Labels, neighbour counts, roots and cluster numbers equal the
    restatement's.  Restatement: under 0.1 s on the CPU."""
    clouds, eps, mp, ref = W.dbscan()
    assert len(clouds) == B > 256 and sum((len(P) + 255) // 256 for P in clouds) >= 257
    assert sum(r[3] for r in ref) > 256 and sum(int((r[0] == -1).sum()) for r in ref) > 256  # clusters and noise
    got = run_dbscan(clouds, eps, mp)
    for i in range(B):
        check_dbscan(got[i], ref[i], "cloud %d" % i)
    for i in EDGE:
        assert blob(run_dbscan([clouds[i]], eps[i], mp[i])[0]) == blob(got[i]), i


# ---- farthest-point down-sampling -----------------------------------------------------------------------------------
def test_farthest_point_down_sampling():
    """The resident map (one workgroup per resident cloud: 210 of them, the clouds with K = 0 and the empty ones left
    out) and the block map of the four clouds above the capacity (164 blocks, the clouds at 0, 256, 257 and 319), both
    built per call; then every cloud streamed (fps_resident_max 0: all 320 in the block map), which must give the same
    bytes.  Indices and both distance outputs equal the restatement's.  Restatement: under 0.1 s on the CPU."""
    clouds, K, start, ref = W.fps()
    assert len(clouds) == B > 256 and fps_capacity() == RP.WIDE_CAPACITY
    assert [i for i in range(B) if len(clouds[i]) > RP.WIDE_CAPACITY] == list(RP.WIDE_LARGE)
    assert sum(1 for P, k in zip(clouds, K) if 0 < len(P) <= RP.WIDE_CAPACITY and k) > 128
    got = fps_both_routes(clouds, K, start)
    for i in range(B):
        if K[i] == 0:
            assert len(got[i][0]) == 0 and len(got[i][1]) == 0 and (got[i][2] == 0).all(), i
            continue
        assert np.array_equal(got[i][0], ref[i][0]), i
        same_fps(got[i], ref[i], "cloud %d" % i)
    for i in EDGE:
        same_fps(run_fps([clouds[i]], K[i], start[i])[0], got[i], "cloud %d alone" % i)


# ---- RGB-D unprojection and projection ------------------------------------------------------------------------------
def test_rgbd_unprojection_and_projection():
    """Unprojection: d_tile_frame and d_tile_prob over more than 256 tiles of 320 frames and rgbd_scan_kernel (one
    workgroup per frame) at frames up to 319 -- the frame list of tests/rgbd_reference.py in turn: 1 x 1, 7 x 5 at
    strides 1, 2, 3, 64 x 4, 257 x 1, 65 x 9, the empty frames, uint16 and float32 depth, every colour variant.
    Projection of 320 small clouds, the race for a pixel (1 000 points on one) having one winner, run twice.  Every
    output equals the restatement's bit for bit.  Restatement: under 0.1 s on the CPU."""
    frames, clouds, _, _ = W.rgbd()
    ucases = RG.unproject_cases()
    assert len(frames) == len(clouds) == B > 256
    assert sum((ucases[k][1].size + RG.TILE - 1) // RG.TILE for k in frames if ucases[k][3].stride == 1) > 256
    got = unproject(frames)
    check_unprojection(frames, got, "320 frames")
    assert sum(len(r) for r in got) > 10000
    for i in EDGE:
        alone = unproject([frames[i]])[0]
        assert blob((alone.points, alone.colors, alone.pixels)) == blob((got[i].points, got[i].colors, got[i].pixels)), i
    first = project(clouds)
    check_projection(clouds, first, "320 clouds")
    again = project(clouds)
    for i in range(B):
        assert blob((first[i].depth, first[i].color, first[i].index, first[i].n_hit)) == \
            blob((again[i].depth, again[i].color, again[i].index, again[i].n_hit)), i
    for i in EDGE:
        alone = project([clouds[i]])[0]
        assert blob((alone.depth, alone.color, alone.index, alone.n_hit)) == \
            blob((first[i].depth, first[i].color, first[i].index, first[i].n_hit)), i


# ---- RGB-D odometry -------------------------------------------------------------------------------------------------
def odometry_fields(r):
    t = r.trace
    return (r.success, r.count, r.iterations, r.transformation, r.information, t.level, t.executed, t.count, t.failed,
            t.e, t.A, t.g, t.pose)


def test_rgbd_odometry_and_its_pyramid_stage():
    """blk_pair ("the blocks of level 0 of all pairs, then level 1, ...", with level_blk0 and level_nblk) over 1 300
    blocks at level 0 and more than 256 at every level, the per-pair partial ranges at part_off, and odo_finish_kernel
    (one workgroup per pair) at pairs up to 319; the cases 4x4, 8x8, 37x29, no_correspondence, f32_specials and
    big_init in turn (options (3, 2, 2)) with the pair whose system is singular at 255 and 257.  Results and traces
    equal the restatement's bit for bit, and so do the pyramids of the same batch.  Restatement: 0.1 s on the CPU."""
    names, ref = W.odometry()
    assert len(names) == B > 256 and [names[i] for i in ROD.WIDE_SINGULAR] == ["singular_3_levels"] * 2
    assert not ref["singular_3_levels"].success and ref["singular_3_levels"].trace[0]["failed"] == 1
    assert sum(ref[n].success for n in names) > 128
    cs = [ROD.cases()[n] for n in names]
    src, tgt = (list(v) for v in zip(*[odo_images(c.pair) for c in cs]))
    K, init = [odo_intrinsic(c.pair) for c in cs], [c.pair.odo_init for c in cs]
    opt = odo_option(cs[0].opt)
    got = tp.compute_rgbd_odometry_batch(src, tgt, K, init, [odo_jacobian(c.pair) for c in cs], opt, return_trace=True)
    for i in range(B):
        check_odometry(got[i], names[i])
    failed = got[255]
    assert not failed.success and odo_same(failed.transformation, np.eye(4)) and not failed.information.any()
    for i in EDGE:
        alone = tp.compute_rgbd_odometry_batch([src[i]], [tgt[i]], [K[i]], [init[i]], [odo_jacobian(cs[i].pair)], opt,
                                               return_trace=True)[0]
        assert blob(odometry_fields(alone)) == blob(odometry_fields(got[i])), i
    pyramids = tp.rgbd_odometry_pyramid_batch(src, tgt, K, init, opt)
    for i in range(B):
        want = ref[names[i]].levels
        assert len(pyramids[i]) == len(want), i
        for l, (g, w) in enumerate(zip(pyramids[i], want)):
            for plane in ("I_s", "I_t", "D_s", "D_t", "I_t_dx", "I_t_dy", "D_t_dx", "D_t_dy"):
                assert np.array_equal(odo_bits(g[plane]), odo_bits(w[plane])), (i, names[i], l, plane)
            assert odo_same(g["XYZ"], np.stack([w["X"], w["Y"], w["Z"]], axis=2)), (i, names[i], l, "XYZ")
    for i in EDGE:
        alone = tp.rgbd_odometry_pyramid_batch([src[i]], [tgt[i]], [K[i]], [init[i]], opt)[0]
        assert blob(alone) == blob(pyramids[i]), i


# ---- the ICP entry that estimates its target normals (it takes the batch width like the entries above it) ------------
def test_icp_with_normals_estimated_inside_the_call():
    """teaser_hip_icp_batch_auto over the 300 problems of tests/test_gpu_batch_width.py: the front-end's own comparison
    (tests/test_gpu_normals.py) is bit equality with the two calls it stands for, estimate_normals_batch and then
    point-to-plane ICP on those normals, both of which that file compares with their restatements at this width."""
    srcs, dsts = icp_problems()
    n = len(srcs)
    assert n > 257
    searches = [tp.KDTreeSearchParamKNN(10) if i % 2 else tp.KDTreeSearchParamHybrid(0.4, 20) for i in range(n)]
    plane = [tp.TransformationEstimationPointToPlane()] * n
    crit = tp.ICPConvergenceCriteria(max_iteration=5)
    auto = tp.registration_icp_batch(srcs, dsts, 0.3, criteria=crit, estimation_methods=plane, target_normals=searches)
    normals = tp.estimate_normals_batch(dsts, searches)
    two = tp.registration_icp_batch(srcs, dsts, 0.3, criteria=crit, estimation_methods=plane, target_normals=normals)
    for i in range(n):
        assert same_icp_bits(auto[i], two[i]) and auto[i].transformation.tobytes() == two[i].transformation.tobytes(), i
    assert sum(r.iterations >= 2 and r.fitness > 0.5 for r in auto) > n // 2
    for i in (0, 63, 64, 65, 255, 256, 257, n - 1):
        alone = tp.registration_icp(srcs[i], dsts[i], 0.3, np.eye(4), plane[i], crit, target_normals=searches[i])
        assert same_icp_bits(alone, auto[i]) and alone.transformation.tobytes() == auto[i].transformation.tobytes(), i
