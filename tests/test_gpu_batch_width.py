"""Every batched front-end on the MI355X with more than 256 clouds and more than 256 point blocks in one call, against
the numpy restatements (tests/voxel_reference.py, outlier_reference.py, normals_reference.py, keypoints_reference.py),
with the comparisons the front-ends' own test files use and no tolerance of its own.

The kernels that give one thread to a cloud (vox_summary, icp_stat_reduce_kernel<0/1>, iss_res_reduce_kernel,
icp_live_kernel, icp_finalize_kernel) launch (batch + 255) / 256 blocks of 256: a wrong blockIdx.x * 256 term shows only
from cloud 256 on.  The kernels that give one thread to a 256-point block of the packed clouds
(icp_stat_block_kernel<0/1>, iss_res_block_kernel) need more than 256 such blocks for the same reason, and the block
maps (blk_prob, tblk_prob, blk_off, tblk_off) then hold hundreds of clouds.  One shared batch of 320 small clouds serves
all of it; clouds 0, 255, 256, 257 and 319 are also compared with the same cloud called alone (tobytes equality).

The last test is about the handle, not the width: the calls of every kind on the ICP handle share its buffers and the
host scaffold of csrc/icp_host.h, so they are run one after the other on ONE handle, in both orders, and compared bit
for bit with the same calls on fresh handles."""
import importlib

import numpy as np
import pytest

import keypoints_reference as RK
import normals_reference as RN
import outlier_reference as RO
import voxel_reference as RV
from test_gpu_icp import same_bits
from test_gpu_keypoints import check as check_iss, run as run_iss
from test_gpu_normals import check as check_normals, reference as normals_reference
from test_gpu_voxel import assert_bits
from util import ROOT  # noqa: F401  (the suite's way to the repository root: the package is imported from there)

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")
Hybrid, KNN = tp.KDTreeSearchParamHybrid, tp.KDTreeSearchParamKNN

B = RN.WIDE_BATCH
EDGE = (0, 255, 256, 257, B - 1)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


@pytest.fixture(scope="module")
def batch():
    clouds = RN.wide_batch()
    assert len(clouds) == B > 256
    return clouds


def cyc(values, i):
    return values[i % len(values)]


def same_bytes(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def test_voxel_down_sample_batch(batch):
    """vox_summary at b >= 256 and vox_trace's summary[2 * b].  Restatement of the 320 clouds: under 0.1 s on the CPU."""
    vs = [cyc((0.05, 0.1, 0.3), i) for i in range(B)]
    got = tp.voxel_down_sample_batch(batch, vs, return_counts=True, return_trace=True)
    for X, v, g in zip(batch, vs, got):
        assert_bits(g, RV.voxel_down_sample(X, v))
    for i in EDGE:
        assert same_bytes(tp.voxel_down_sample(batch[i], vs[i], return_counts=True, return_trace=True), got[i]), i


def test_self_knn_batch_with_both_list_capacities_and_both_routes(batch):
    """k <= 32 in one call (the short lists), k up to 100 in another (the long ones); each at knn_ring_cap 4 and at 0,
    where every query goes through the whole-cloud scan.  Restatement: 0.1 s on the CPU for both calls."""
    total = sum(len(X) for X in batch)
    for ks in ((1, 5, 32), (1, 5, 32, 33, 100)):
        kk = [cyc(ks, i) for i in range(B)]
        ref = [RO.self_knn(X, k) for X, k in zip(batch, kk)]
        try:
            for cap in (4, 0):
                tp.set_icp_option("knn_ring_cap", cap)
                got = tp.self_knn_batch(batch, kk, return_distance=True)
                if cap == 0:
                    assert tp.get_icp_option("knn_fallbacks") == total
                for i, ((idx, d2), (ridx, rd2)) in enumerate(zip(got, ref)):
                    assert idx.dtype == np.int32 and np.array_equal(idx, ridx), (cap, i)
                    assert RO.bits_equal(d2, rd2), (cap, i)
                for i in EDGE:
                    assert same_bytes(tp.self_knn(batch[i], kk[i], return_distance=True), got[i]), (cap, i)
        finally:
            tp.set_icp_option("knn_ring_cap", 4)


def test_remove_statistical_outlier_batch(batch):
    """icp_stat_reduce_kernel<0/1> at p >= 256 and icp_stat_block_kernel<0/1> at t >= 256 (the batch has 280 point
    blocks).  Restatement: 0.2 s on the CPU."""
    nb = [cyc((3, 20, 40), i) for i in range(B)]
    ratio = [cyc((0.5, 1.0, 2.0), i // 3) for i in range(B)]  # every pairing of the two cycles
    got = tp.remove_statistical_outlier_batch(batch, nb, ratio, return_stats=True)
    kept = 0
    for i, (X, (pts, ind, st)) in enumerate(zip(batch, got)):
        ref = RO.statistical(X, nb[i], ratio[i])
        assert np.array_equal(ind, np.flatnonzero(ref["keep"])) and np.array_equal(pts, X[ind]), i
        assert RO.bits_equal(st["avg"], ref["avg"]), i
        assert RO.bits_equal([st["mean"], st["std"], st["threshold"]], [ref["mean"], ref["std"], ref["threshold"]]), i
        kept += len(ind)
    assert 0 < kept < sum(len(X) for X in batch)
    for i in EDGE:
        a = tp.remove_statistical_outlier(batch[i], nb[i], ratio[i], return_stats=True)
        assert same_bytes((a[0], a[1], a[2]["avg"]), (got[i][0], got[i][1], got[i][2]["avg"])), i
        assert RO.bits_equal([a[2][k] for k in ("mean", "std", "threshold")],
                             [got[i][2][k] for k in ("mean", "std", "threshold")]), i


def test_remove_radius_outlier_batch(batch):
    """icp_radius_count_kernel and its keep counts over 280 point blocks.  Restatement: under 0.1 s on the CPU."""
    radius = [cyc((0.2, 0.35), i) for i in range(B)]
    nb = [cyc((1, 4), i // 2) for i in range(B)]
    got = tp.remove_radius_outlier_batch(batch, nb, radius, return_counts=True)
    kept = 0
    for i, (X, (pts, ind, cnt)) in enumerate(zip(batch, got)):
        ref = RO.radius(X, nb[i], radius[i])
        assert np.array_equal(cnt, ref["count"]) and np.array_equal(ind, np.flatnonzero(ref["keep"])), i
        assert np.array_equal(pts, X[ind]), i
        kept += len(ind)
    assert 0 < kept < sum(len(X) for X in batch)
    for i in EDGE:
        assert same_bytes(tp.remove_radius_outlier(batch[i], nb[i], radius[i], return_counts=True), got[i]), i


# The library offers two searches (include/teaser_hip.h, "Normal estimation"): k nearest, and k nearest inside a
# radius.  "radius": the hybrid search with a cap no cloud of the batch reaches (100 > 65 points), so the radius alone
# decides; "hybrid": a cap and a radius that both bind.
SEARCHES = {"knn": lambda i: KNN(cyc((5, 33, 12), i)),
            "radius": lambda i: Hybrid(cyc((0.35, 0.5), i), 100).along([0.0, 0.0, 1.0]),
            "hybrid": lambda i: Hybrid(0.3, cyc((10, 40), i)).towards([0.5, 0.5, 5.0])}


@pytest.mark.parametrize("search", sorted(SEARCHES))
def test_estimate_normals_batch(batch, search):
    """One call over the whole batch per search.  Restatement: 2.0 s (knn), 2.2 s (radius), 2.1 s (hybrid) on the CPU."""
    sps = [SEARCHES[search](i) for i in range(B)]
    got = tp.estimate_normals_batch(batch, sps, covariances=True, eigenvalues=True)
    below, fitted = 0, 0
    for i, (X, sp, g) in enumerate(zip(batch, sps, got)):
        ref = normals_reference(X, sp)
        check_normals(g, ref, "%s, cloud %d" % (search, i))
        below += int((ref[3] < 3).sum())
        fitted += int((ref[3] >= 3).sum())
    assert below > 0 and fitted > 1000  # both the filled-in normals and the fitted ones occur
    for i in EDGE:
        assert same_bytes(tp.estimate_normals(batch[i], sps[i], covariances=True, eigenvalues=True), got[i]), i


def test_compute_iss_keypoints_batch(batch):
    """Odd clouds with automatic radii: iss_res_reduce_kernel at p >= 256; the grid ids run to 2 * 320 - 1, ten bits
    above the cell bits.  Restatement: 2.6 s on the CPU."""
    params = RK.wide_batch_params(B)
    bits, cell_bits, id_bits, _ = RK.key_bits(batch, [p.get("salient_radius", 0.0) for p in params],
                                              [p.get("non_max_radius", 0.0) for p in params], details=True)
    assert id_bits == 10 and cell_bits >= 3 and bits <= 63
    got = run_iss(batch, params)
    keypoints = 0
    for i, (X, p, g) in enumerate(zip(batch, params, got)):
        keypoints += int(check_iss(g, X, p, "cloud %d" % i)["keep"].sum())
    assert keypoints > 0
    for i in EDGE:
        alone = run_iss([batch[i]], [params[i]])[0]
        assert same_bytes((alone[0], alone[1]["saliency"], alone[1]["count"]),
                          (got[i][0], got[i][1]["saliency"], got[i][1]["count"])), i
        assert RO.bits_equal([alone[1][k] for k in ("resolution", "salient_radius", "non_max_radius")],
                             [got[i][1][k] for k in ("resolution", "salient_radius", "non_max_radius")]), i


def test_iss_resolution_over_more_than_256_point_blocks(batch):
    """Only the clouds with automatic radii and two or more points get resolution blocks: 120 in the test above.  Here
    every cloud of the batch and of its first 80 again asks for them, 300 blocks: iss_res_block_kernel at t >= 256.
    min_neighbors above every cloud's size: the resolution, the radii and both counts are compared, no covariance is
    fitted.  400 clouds, as in the test below.  Restatement: 0.4 s on the CPU."""
    clouds = batch + batch[:80]
    assert sum((len(X) + 255) // 256 for X in clouds if len(X) >= 2) >= 257
    p = dict(min_neighbors=1000)
    got = run_iss(clouds, [p] * len(clouds))
    counted = 0
    for i, (X, g) in enumerate(zip(clouds, got)):
        ref = check_iss(g, X, p, "cloud %d" % i)
        counted += int(ref["count"].sum())
        assert not ref["keep"].any() and (len(X) < 2 or ref["radii"][0] > 0)
    assert counted > sum(len(X) for X in clouds)  # neighbours were found with the automatic radii
    for i in (255, 256, 257, len(clouds) - 1):
        alone = run_iss([clouds[i]], [p])[0]
        assert same_bytes((alone[1]["count"], alone[1]["resolution"]), (got[i][1]["count"], got[i][1]["resolution"])), i


def test_400_clouds_reach_past_one_and_a_half_blocks_of_threads(batch):
    """With 320 clouds a per-cloud kernel whose second block started at 128 instead of 256 would still write every
    cloud (128 .. 383) with the right value; with 400 clouds it leaves 384 .. 399 unwritten.  Voxel down-sampling and
    statistical removal over the batch and its first 80 clouds again.  Restatement: 0.3 s on the CPU."""
    clouds = batch + batch[:80]
    assert len(clouds) > 256 + 128 and len(clouds[-1]) > 0 and len(clouds[385]) > 0
    vs = [cyc((0.05, 0.1, 0.3), i) for i in range(len(clouds))]
    for X, v, g in zip(clouds, vs, tp.voxel_down_sample_batch(clouds, vs, return_counts=True, return_trace=True)):
        assert_bits(g, RV.voxel_down_sample(X, v))
    nb = [cyc((3, 20, 40), i) for i in range(len(clouds))]
    got = tp.remove_statistical_outlier_batch(clouds, nb, 1.0, return_stats=True)
    for i, (X, (pts, ind, st)) in enumerate(zip(clouds, got)):
        ref = RO.statistical(X, nb[i], 1.0)
        assert np.array_equal(ind, np.flatnonzero(ref["keep"])) and RO.bits_equal(st["avg"], ref["avg"]), i
        assert RO.bits_equal([st["mean"], st["std"], st["threshold"]], [ref["mean"], ref["std"], ref["threshold"]]), i


def icp_problems(n_problems=300):
    """Per problem a 40 to 70 point cube cloud as the target and a rigidly moved copy as the source."""
    rng = np.random.default_rng(77)
    srcs, dsts = [], []
    for k in range(n_problems):
        Q = RN.cube(40 + k % 31, 5000 + k)
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        th = np.deg2rad(rng.uniform(1.0, 4.0))
        Rm = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        srcs.append(np.ascontiguousarray((Q - 0.5) @ Rm.T + 0.5 + rng.normal(0, 0.01, 3)))
        dsts.append(Q)
    return srcs, dsts


@pytest.mark.parametrize("method", ["point", "plane", "gicp"])
def test_registration_icp_batch_with_300_problems(method):
    """icp_live_kernel and icp_finalize_kernel at p >= 256.  Problems 0, 255, 256, 257 and 299 against the same problem
    solved alone (alone against the restatement: tests/test_gpu_icp*.py)."""
    srcs, dsts = icp_problems()
    n = len(srcs)
    assert n > 257 and len({len(q) for q in dsts}) > 8
    crit = tp.ICPConvergenceCriteria(max_iteration=5)
    none = [None] * n
    est, normals, cs, ct = None, none, none, none
    if method == "plane":
        est = tp.TransformationEstimationPointToPlane()
        rng = np.random.default_rng(78)
        normals = [rng.normal(size=q.shape) for q in dsts]
        normals = [v / np.linalg.norm(v, axis=1, keepdims=True) for v in normals]
    if method == "gicp":
        est = tp.TransformationEstimationForGeneralizedICP()
        both = tp.estimate_covariances_batch(srcs + dsts, 0.4, 20)  # 600 clouds in one call
        cs, ct = both[:n], both[n:]
        for i in (0, 255, 256, 257, n - 1, n + 256, 2 * n - 1):
            assert tp.estimate_covariances((srcs + dsts)[i], 0.4, 20).tobytes() == both[i].tobytes(), i
    kw = {} if est is None else dict(estimation_methods=[est] * n, target_normals=normals, source_covariances=cs,
                                     target_covariances=ct)
    got = tp.registration_icp_batch(srcs, dsts, 0.3, inits=np.eye(4), criteria=crit, **kw)
    assert len(got) == n
    assert all(g.iterations >= 1 and np.isfinite(g.transformation).all() for g in got)
    assert sum(g.fitness > 0.5 for g in got) > n // 2
    for i in (0, 255, 256, 257, n - 1):
        alone = tp.registration_icp(srcs[i], dsts[i], 0.3, np.eye(4), est, crit, target_normals=normals[i],
                                    source_covariances=cs[i], target_covariances=ct[i])
        assert same_bits(got[i], alone), i
        assert not np.array_equal(alone.transformation, np.eye(4)), i


def blob(x):
    """Every number of a result as bytes, in a fixed order."""
    if isinstance(x, dict):
        return [(k, blob(x[k])) for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [blob(v) for v in x]
    if hasattr(x, "__dict__"):
        return blob(vars(x))
    return np.asarray(x).tobytes()


def test_calls_of_every_kind_on_one_handle_equal_the_same_calls_on_fresh_handles():
    """Keypoints with automatic radii, radius removal, normals with k-NN search, self k-NN, statistical removal,
    covariances and the ICP entry that estimates its normals, then the same list backwards, all on one handle; every
    call over clouds of 300, 0, 65, 1 and 257 points (the largest first: the later clouds meet grown buffers).  A call
    that left something behind in a shared buffer, or sized one for itself alone, shows as a bit that differs from the
    same call on a handle of its own -- and so does "knn_fallbacks", which the far point of the first cloud makes
    non-zero.  Radius removal and covariance estimation run no k-NN search and by the contract leave the option alone
    (include/teaser_hip.h, "Options of an ICP handle"): after them it must still hold what the last call that reports
    it left, which is 0 on a fresh handle.  No restatement: 14 + 7 small calls, well under a second."""
    clouds = [RN.cube(n, 300 + n) for n in (300, 0, 65, 1, 257)]
    clouds[0][7] = 1000.0  # rings 0 .. 3 of its grid hold none of its neighbours: the whole-cloud route serves it
    rng = np.random.default_rng(12)
    srcs = [X + rng.normal(0, 0.01, X.shape) for X in clouds]
    plane = tp.TransformationEstimationPointToPlane()
    ests = [plane if len(X) else None for X in clouds]
    searches = [KNN(10) if len(X) else None for X in clouds]
    crit = tp.ICPConvergenceCriteria(max_iteration=5)
    calls = [
        ("keypoints", True, lambda: tp.compute_iss_keypoints_batch(clouds, return_saliency=True)),
        ("radius", False, lambda: tp.remove_radius_outlier_batch(clouds, 3, 0.2, return_counts=True)),
        ("normals", True, lambda: tp.estimate_normals_batch(clouds, KNN(10), covariances=True, eigenvalues=True)),
        ("self_knn", True, lambda: tp.self_knn_batch(clouds, 7, return_distance=True)),
        ("statistical", True, lambda: tp.remove_statistical_outlier_batch(clouds, 8, 1.5, return_stats=True)),
        ("covariances", False, lambda: tp.estimate_covariances_batch(clouds, 0.3, 20)),
        ("icp_auto", True, lambda: tp.registration_icp_batch(srcs, clouds, 0.3, criteria=crit, estimation_methods=ests,
                                                             target_normals=searches)),
    ]  # (name, whether the call reports "knn_fallbacks", the call)

    def run(fn):
        return blob(fn()), tp.get_icp_option("knn_fallbacks")

    fresh = {}
    for name, reports, fn in calls:
        tp.icp._cache.release()  # the next call opens a new handle
        fresh[name] = run(fn)
        assert reports or fresh[name][1] == 0, name
    assert fresh["self_knn"][1] >= 1 and fresh["statistical"][1] >= 1
    tp.icp._cache.release()
    last = 0  # "knn_fallbacks" of the last call on this handle that reports it
    for name, reports, fn in calls + calls[::-1]:
        got = run(fn)
        want = fresh[name][1] if reports else last
        assert got[1] == want, "%s: knn_fallbacks %d, expected %d" % (name, got[1], want)
        assert got[0] == fresh[name][0], name
        last = got[1]
