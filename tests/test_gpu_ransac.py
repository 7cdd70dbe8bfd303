"""RANSAC registration on the GPU against the contract of include/teaser_hip.h, stage by stage through
teaser_hip_ransac_trials_batch and then as the full call, on the fixture of tests/golden/make_ransac_golden.py:
  1  samples and edge-length flags equal the restatement's for every trial, at launch sizes around the wave and block
     edges and at a first trial above 2^32
  2  T per trial within 16 max(A, 2^-52 cond) of the 50-digit Kabsch pose wherever cond <= 1e3 (the rule of
     tests/test_gpu_icp_step.py); the rest rigid and maximising
  3  distance flags, count and sum d2 equal the restatement evaluated on the device's own T, bit for bit
  4  the full call equals the contract's loop run by the restatement over the device's per-trial records
  5  the exact-pose case is recovered
  6  the bits do not depend on chunk_trials, on the batch around a problem or on the run
  7  defaults and refusals
Measured once on an MI355X (test 2 prints them): the largest |dT| / bar is 0.096 (e3), 0.15 (n48), 0.18 (e255), 0.16
(n256), 0.18 (n257); the largest |dT| among the trials with cond <= 1e3 is 3.4e-14."""
import importlib
import os

import numpy as np
import pytest

import ransac_reference as RR
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(ROOT, "tests", "golden", "ransac_golden.npz"))
CASES = [str(n) for n in G["trial_cases"]]
TRIALS = int(G["trials"])
COND_MAX = 1e3


def case(name):
    r, s, d = G[name + "/params"]
    return dict(P=G[name + "/P"], Q=G[name + "/Q"], corr=G[name + "/corr"], r=float(r), s=float(s), d=float(d),
                seed=int(G[name + "/seed"][0]), ransac_n=int(G[name + "/ransac_n"]))


def checkers_of(c, on=True):
    out = []
    if on and c["s"] > 0:
        out.append(tp.CorrespondenceCheckerBasedOnEdgeLength(c["s"]))
    if on and c["d"] > 0:
        out.append(tp.CorrespondenceCheckerBasedOnDistance(c["d"]))
    return out


_stage = {}


def stage(name, first, n, checkers=True):
    """The device's per-trial records, once per process."""
    key = (name, first, n, checkers)
    if key not in _stage:
        c = case(name)
        _stage[key] = tp.ransac_trials_batch([c["P"]], [c["Q"]], [c["corr"]], c["r"], first, n, None, c["ransac_n"],
                                             checkers_of(c, checkers), c["seed"])[0]
    return _stage[key]


def restated(name, first, n, checkers, T):
    c = case(name)
    return RR.trial_records(c["P"], c["Q"], c["corr"], c["r"], first, n, c["ransac_n"], c["s"] if checkers else 0.0,
                            c["d"] if checkers else 0.0, c["seed"], T=T)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1 ----
@pytest.mark.parametrize("first,n", [(0, 63), (0, 64), (0, 65), (0, 255), (0, 256), (0, 257), (0, 2048),
                                     ((1 << 32) + 12345, 257)])
@pytest.mark.parametrize("name", CASES)
def test_samples_and_edge_length_flags_equal_the_restatement(name, first, n):
    dev = stage(name, first, n)
    ref = restated(name, first, n, True, dev["transformation"])
    assert np.array_equal(dev["samples"], ref["samples"])
    assert np.array_equal(dev["flags"] & RR.FLAG_EDGE, ref["flags"] & RR.FLAG_EDGE)
    failed = (dev["flags"] & RR.FLAG_EDGE) == 0
    assert np.array_equal(dev["transformation"][failed], np.tile(np.eye(4), (failed.sum(), 1, 1)))  # not estimated
    assert 0 < failed.sum() < n or name == "e3"


# ---- 2 ----
def check_rigid(T):
    assert np.isfinite(T).all() and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    Rm = T[:3, :3]
    assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rm) - 1.0) <= 1e-12


def check_maximiser(T, rec, smp_row):
    """Where the rotation is not unique or ill-conditioned: a proper rotation that maximises tr(R H), with its t."""
    check_rigid(T)
    mp, mq, H = RR.cross_covariance(rec, smp_row)
    Rm = T[:3, :3]
    assert np.abs(T[:3, 3] - (mq - Rm @ mp)).max() <= 1e-12 * max(np.abs(mp).max(), np.abs(mq).max(), 1.0)
    if not H.any():
        assert np.array_equal(Rm, np.eye(3))
        return
    U, sv, Vt = np.linalg.svd(H)
    d = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    RH = Rm @ H
    assert np.abs(RH - RH.T).max() <= 1e-12 * sv[0]
    assert abs(np.trace(RH) - (sv[0] + sv[1] + d * sv[2])) <= 1e-12 * sv[0]


@pytest.mark.parametrize("name", CASES)
def test_estimate_matches_the_50_digit_pose_of_every_trial(name):
    dev = stage(name, 0, TRIALS, False)
    assert (dev["flags"] == 7).all()  # checkers off: every trial estimated and scored
    c = case(name)
    rec = RR.records_of(c["P"], c["Q"], c["corr"])
    gT, cond, A = G[name + "/gT"], G[name + "/cond"].astype(np.float64), G[name + "/A"].astype(np.float64)
    good = cond <= COND_MAX
    assert good.mean() >= 0.75 or name == "e3"  # e3: 21 of its 27 sample triples repeat a pair
    err = np.linalg.norm(dev["transformation"][:, :3].reshape(TRIALS, 12) - gT, axis=1)
    bar = 16.0 * np.maximum(A, 2.0 ** -52 * cond)
    worst = (err[good] / bar[good]).max()
    print("%s: %d of %d trials with cond <= 1e3; largest |dT| / bar = %.3g (|dT| up to %.3g)" % (
        name, good.sum(), TRIALS, worst, err[good].max()))
    for q in np.nonzero(good)[0][:64]:
        check_rigid(dev["transformation"][q])
    assert (err[good] <= bar[good]).all()
    for q in np.nonzero(~good)[0]:
        check_maximiser(dev["transformation"][q], rec, dev["samples"][q])


# ---- 3 ----
@pytest.mark.parametrize("checkers", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_distance_flags_count_and_sum_equal_the_restatement_on_the_devices_t(name, checkers):
    dev = stage(name, 0, TRIALS, checkers)
    ref = restated(name, 0, TRIALS, checkers, dev["transformation"])
    assert np.array_equal(dev["flags"], ref["flags"])
    assert np.array_equal(dev["count"], ref["count"])
    assert np.array_equal(bits(dev["sum_d2"]), bits(ref["sum_d2"]))
    scored = (dev["flags"] & RR.FLAG_SCORED) != 0
    assert scored.any() and (dev["count"][~scored] == 0).all() and (dev["sum_d2"][~scored] == 0).all()
    if checkers and name != "e3":
        assert (~scored).any()


def test_a_problem_with_fewer_pairs_than_samples_draws_nothing():
    c2, c = case("tiny2"), case("n48")
    out = tp.ransac_trials_batch([c["P"], c2["P"]], [c["Q"], c2["Q"]], [c["corr"], c2["corr"]], c["r"], 0, 100,
                                 seed=[c["seed"], c2["seed"]])
    assert (out[1]["samples"] == -1).all() and not out[1]["flags"].any() and not out[1]["count"].any()
    assert np.array_equal(out[1]["transformation"], np.tile(np.eye(4), (100, 1, 1)))
    alone = stage("n48", 0, TRIALS, False)
    for k in ("samples", "flags", "count"):
        assert np.array_equal(out[0][k], alone[k][:100])
    assert np.array_equal(bits(out[0]["transformation"]), bits(alone["transformation"][:100]))


# ---- 4 ----
def full_call(name, chunk=None, **kw):
    c = case(name)
    max_iteration, confidence = int(G[name + "/criteria"][0]), float(G[name + "/criteria"][1])
    before = tp.get_ransac_option("chunk_trials")
    try:
        if chunk:
            tp.set_ransac_option("chunk_trials", chunk)
        return tp.registration_ransac_based_on_correspondence(
            c["P"], c["Q"], c["corr"], c["r"], None, c["ransac_n"], checkers_of(c),
            tp.RANSACConvergenceCriteria(max_iteration, confidence), c["seed"], **kw)
    finally:
        tp.set_ransac_option("chunk_trials", before)


@pytest.mark.parametrize("chunk", [64, 256, None])
@pytest.mark.parametrize("name", ["early", "full"])
def test_full_call_equals_the_sequential_loop_over_the_devices_records(name, chunk):
    c = case(name)
    max_iteration, confidence = int(G[name + "/criteria"][0]), float(G[name + "/criteria"][1])
    dev = stage(name, 0, max_iteration)
    want = RR.loop(lambda first, n: {k: v[first:first + n] for k, v in dev.items()}, len(c["corr"]), c["ransac_n"],
                   max_iteration, confidence)
    got = full_call(name, chunk)
    print("%s: trials %d, valid %d, best trial %d, %d inliers" % (name, got.trials, got.valid_trials, got.best_trial,
                                                                  len(got.correspondence_set)))
    assert (got.best_trial, got.trials, got.valid_trials) == (want["best_trial"], want["trials"], want["valid_trials"])
    assert bits(got.fitness) == bits(want["fitness"]) and bits(got.inlier_rmse) == bits(want["inlier_rmse"])
    assert np.array_equal(bits(got.transformation), bits(dev["transformation"][got.best_trial]))
    inl = RR.score(got.transformation[None], RR.records_of(c["P"], c["Q"], c["corr"]), c["r"])[2][0]
    assert np.array_equal(got.correspondence_set, c["corr"][inl]) and len(got.correspondence_set) == want["count"]
    assert 0 < got.valid_trials < got.trials
    if name == "early":  # stops by the confidence rule strictly between two chunk edges, past the first chunk of 64
        assert 64 < got.trials < max_iteration and got.trials % 64 != 0
    else:
        assert got.trials == max_iteration


# ---- 5 ----
def test_exact_pose_case_is_recovered():
    c = case("e255")
    got = tp.registration_ransac_based_on_correspondence(c["P"], c["Q"], c["corr"], c["r"], ransac_n=3,
                                                         criteria=tp.RANSACConvergenceCriteria(TRIALS, 0.999),
                                                         seed=c["seed"])
    q = got.best_trial
    assert 0 <= q < got.trials <= TRIALS and len(got.correspondence_set) >= G["e255/planted"].sum()
    bar = 16.0 * max(float(G["e255/A"][q]), 2.0 ** -52 * float(G["e255/cond"][q]))
    err = np.linalg.norm(got.transformation - G["e255/T_true"])
    print("e255: best trial %d, %d inliers, |T - truth| %.3g, bar %.3g" % (q, len(got.correspondence_set), err, bar))
    assert err <= bar


# ---- 6 ----
def result_bits(r):
    return (r.transformation.tobytes(), np.float64(r.fitness).tobytes(), np.float64(r.inlier_rmse).tobytes(),
            r.best_trial, r.trials, r.valid_trials, r.correspondence_set.tobytes())


def mixed_batch():
    names = ["n257", "n48", "e3", "tiny2"]
    cs = [case(n) for n in names]
    P = [c["P"] for c in cs] + [np.zeros((0, 3))]
    Q = [c["Q"] for c in cs] + [np.zeros((0, 3))]
    corr = [c["corr"] for c in cs] + [np.zeros((0, 2), dtype=np.int32)]
    checkers = [checkers_of(c) for c in cs] + [[]]
    kw = dict(max_correspondence_distance=[c["r"] for c in cs] + [0.1], ransac_n=3, checkers=checkers,
              criteria=[tp.RANSACConvergenceCriteria(700, conf) for conf in (0.999, 1.0, 0.999, 0.999, 0.999)],
              seed=[c["seed"] for c in cs] + [9])
    return P, Q, corr, kw


def test_bits_do_not_depend_on_chunk_batch_or_run():
    P, Q, corr, kw = mixed_batch()
    before = tp.get_ransac_option("chunk_trials")
    assert before == 4096
    runs = {}
    try:
        for chunk in (64, 256, before):
            tp.set_ransac_option("chunk_trials", chunk)
            runs[chunk] = [result_bits(r) for r in tp.registration_ransac_based_on_correspondence_batch(P, Q, corr, **kw)]
        again = [result_bits(r) for r in tp.registration_ransac_based_on_correspondence_batch(P, Q, corr, **kw)]
        alone = []
        for b in range(len(P)):
            one = dict(kw, max_correspondence_distance=kw["max_correspondence_distance"][b], checkers=kw["checkers"][b],
                       seed=kw["seed"][b], criteria=kw["criteria"][b])
            alone.append(result_bits(tp.registration_ransac_based_on_correspondence(P[b], Q[b], corr[b], **one)))
    finally:
        tp.set_ransac_option("chunk_trials", before)
    assert runs[64] == runs[256] == runs[before] == again == alone
    res = tp.registration_ransac_based_on_correspondence_batch(P, Q, corr, **kw)
    assert res[0].best_trial >= 0 and 0 < res[0].trials < 700  # one problem stops early ...
    assert res[1].best_trial >= 0 and res[1].trials == 700     # ... one crosses every chunk edge (confidence 1) ...
    assert res[2].best_trial >= 0 and res[2].trials == res[2].best_trial + 1  # ... e3 stops at its first full fit
    for r in res[3:]:  # ncorr = 2 and the empty problem: the start
        assert r.best_trial == -1 and r.trials == 0 and np.array_equal(r.transformation, np.eye(4))
    with pytest.raises(tp.TeaserHipError, match="chunk_trials"):
        tp.set_ransac_option("chunk_trials", 63)
    with pytest.raises(tp.TeaserHipError, match="chunk_trials"):
        tp.set_ransac_option("chunk_trials", 65537)


# ---- 7 ----
def test_defaults_where_no_trial_can_run():
    c, c2 = case("n48"), case("tiny2")
    for r in (tp.registration_ransac_based_on_correspondence(c2["P"], c2["Q"], c2["corr"], c2["r"], seed=3),
              tp.registration_ransac_based_on_correspondence(c["P"], c["Q"], c["corr"], c["r"], seed=3,
                                                             criteria=tp.RANSACConvergenceCriteria(0, 0.999))):
        assert np.array_equal(r.transformation, np.eye(4)) and r.fitness == 0.0 and r.inlier_rmse == 0.0
        assert (r.best_trial, r.trials, r.valid_trials) == (-1, 0, 0) and r.correspondence_set.shape == (0, 2)


def refused(match, edit=None, raw=None):
    c = case("n48")
    P, Q, corr = [c["P"].copy(), c["P"].copy()], [c["Q"].copy(), c["Q"].copy()], [c["corr"].copy(), c["corr"].copy()]
    kw = dict(max_correspondence_distance=[c["r"], c["r"]], ransac_n=[3, 3], checkers=[[], []],
              criteria=[tp.RANSACConvergenceCriteria(10, 0.9), tp.RANSACConvergenceCriteria(10, 0.9)], seed=[1, 2])
    if edit:
        edit(P, Q, corr, kw)
    with pytest.raises(tp.TeaserHipError, match=match) as e:
        if raw is None:
            tp.registration_ransac_based_on_correspondence_batch(P, Q, corr, **kw)
        else:
            b, args, keep = tp.ransac._gather(P, Q, corr, kw["max_correspondence_distance"], None, kw["ransac_n"],
                                              kw["checkers"], kw["criteria"], kw["seed"])
            raw(args[6][1])
            out = (tp.ransac.RansacResultC * b)()
            h = tp.ransac._cache.get(-1)
            h.call(h._lib.teaser_hip_ransac_correspondence_batch, b, *args, out, None)
    assert e.value.status == 1 and "(problem 1)" in str(e.value)


def test_every_refusal_names_its_argument_and_its_problem():
    def setkw(key, value):
        return lambda P, Q, corr, kw: kw[key].__setitem__(1, value)

    refused("max_correspondence_distance", setkw("max_correspondence_distance", 0.0))
    refused("max_correspondence_distance", setkw("max_correspondence_distance", float("inf")))
    refused("ransac_n", setkw("ransac_n", 2))
    refused("ransac_n", setkw("ransac_n", 9))
    refused("confidence", setkw("criteria", tp.RANSACConvergenceCriteria(10, 1.5)))
    refused("confidence", setkw("criteria", tp.RANSACConvergenceCriteria(10, float("nan"))))
    refused("max_iteration", setkw("criteria", tp.RANSACConvergenceCriteria(-1, 0.9)))
    refused("edge_length_threshold", setkw("checkers", [tp.CorrespondenceCheckerBasedOnEdgeLength(1.5)]))
    refused("distance_threshold", setkw("checkers", [tp.CorrespondenceCheckerBasedOnDistance(float("inf"))]))
    refused("corr: source index of pair 5", lambda P, Q, corr, kw: corr[1].__setitem__((5, 0), len(P[1])))
    refused("corr: target index of pair 7", lambda P, Q, corr, kw: corr[1].__setitem__((7, 1), -1))
    refused("src has non-finite points", lambda P, Q, corr, kw: P[1].__setitem__((0, 0), np.nan))
    refused("dst has non-finite points", lambda P, Q, corr, kw: Q[1].__setitem__((3, 2), np.inf))
    refused("with_scaling", raw=lambda p: setattr(p, "with_scaling", 1))
    refused("point-to-plane", raw=lambda p: setattr(p, "estimation", 1))
    refused("normal-angle checker", raw=lambda p: setattr(p, "normal_checker", 1))
    # the handle is sound afterwards
    c = case("n48")
    r = tp.registration_ransac_based_on_correspondence(c["P"], c["Q"], c["corr"], c["r"], seed=c["seed"],
                                                       criteria=tp.RANSACConvergenceCriteria(200, 0.999))
    assert r.best_trial >= 0 and r.trials <= 200
