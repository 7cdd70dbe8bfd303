"""Batched point-to-point ICP on the MI355X against the numpy restatement of the contract (tests/icp_reference.py):
same correspondence sets and iteration counts, transforms within 1e-9, fitness / RMSE within 1e-12 relative (far from
the origin: the bars the coordinates' own rounding allows, see test_far_from_the_origin); a problem inside a batch
gives the same bits as alone; invalid arguments are refused with the argument named."""
import ctypes as C
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import icp_reference as R
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose(axis, deg, t):
    T = np.eye(4)
    T[:3, :3] = rot(axis, deg)
    T[:3, 3] = t
    return T


def assert_matches(gpu, ref):
    assert gpu.iterations == ref["iterations"]
    assert np.array_equal(gpu.correspondence_set, ref["correspondence_set"])
    assert np.linalg.norm(gpu.transformation - ref["transformation"]) < 1e-9
    assert abs(gpu.fitness - ref["fitness"]) <= 1e-12 * max(ref["fitness"], 1e-300)
    assert abs(gpu.inlier_rmse - ref["inlier_rmse"]) <= 1e-12 * max(ref["inlier_rmse"], 1e-300)


def same_bits(a, b):
    return (a.transformation.tobytes() == b.transformation.tobytes() and a.fitness == b.fitness and
            a.inlier_rmse == b.inlier_rmse and a.iterations == b.iterations and
            np.array_equal(a.correspondence_set, b.correspondence_set))


def synthetic_pair(seed=11, n=5000):
    rng = np.random.default_rng(seed)
    P = rng.uniform(0, 1, size=(n, 3))
    T_true = pose([0.3, -1, 0.5], 5.0, [0.05, -0.03, 0.02])
    Q = R.apply(T_true, P) + rng.normal(0, 0.003, size=(n, 3))
    k = int(0.8 * n)  # 20 % of the target points have no counterpart in the source
    Q = np.concatenate([Q[:k], rng.uniform(0, 1, size=(n - k, 3))])
    return P, Q, T_true


def test_synthetic_pair_matches_the_restatement():
    P, Q, T_true = synthetic_pair()
    ref = R.registration_icp(P, Q, 0.08, np.eye(4))
    gpu = tp.registration_icp(P, Q, 0.08, np.eye(4))
    assert_matches(gpu, ref)
    assert gpu.fitness > 0.7 and np.linalg.norm(gpu.transformation - T_true) < 0.05


def test_config5_refinement_matches_golden():
    P, Q, r, init = R.config5_problem()
    g = np.load(os.path.join(ROOT, "tests", "golden", "icp_golden.npz"))
    crit = tp.ICPConvergenceCriteria(max_iteration=100)
    gpu = tp.registration_icp(P, Q, r, init, tp.TransformationEstimationPointToPoint(), crit)
    ref = {k: g[k] for k in ("transformation", "correspondence_set")}
    ref.update(fitness=float(g["fitness"]), inlier_rmse=float(g["inlier_rmse"]), iterations=int(g["iterations"]))
    assert_matches(gpu, ref)
    assert gpu.fitness >= float(g["init_fitness"])
    zero = tp.registration_icp(P, Q, r, init, criteria=tp.ICPConvergenceCriteria(max_iteration=0))
    assert zero.iterations == 0 and np.array_equal(zero.transformation, init)
    assert abs(zero.fitness - float(g["init_fitness"])) <= 1e-12 * zero.fitness


def mixed_batch():
    P, Q, r, init = R.config5_problem()
    rng = np.random.default_rng(2024)
    srcs, dsts, rs, inits = [], [], [], []
    for k in range(64):
        T = pose(rng.normal(size=3), rng.uniform(0, 3), rng.normal(0, 0.02, 3)) @ init
        srcs.append(P), dsts.append(Q), rs.append(r * (1.0, 1.5, 2.0)[k % 3]), inits.append(T)
    srcs.append(P[:0]), dsts.append(Q), rs.append(r), inits.append(init)          # n_s = 0
    srcs.append(P), dsts.append(Q[:0]), rs.append(r), inits.append(init)          # n_t = 0
    far = init.copy()
    far[:3, 3] += 100.0
    srcs.append(P), dsts.append(Q), rs.append(r), inits.append(far)               # no correspondence at all
    rng = np.random.default_rng(5)                                                # dense pair: jittered upsampling
    A = np.repeat(P, 48, axis=0) + rng.normal(0, 0.01, size=(48 * len(P), 3))
    B = np.repeat(Q, 50, axis=0) + rng.normal(0, 0.01, size=(50 * len(Q), 3))
    srcs.append(A), dsts.append(B), rs.append(r), inits.append(init)
    return srcs, dsts, rs, inits


def test_batch_is_bit_identical_to_single_runs():
    srcs, dsts, rs, inits = mixed_batch()
    assert len(srcs) >= 68 and len(srcs[-1]) > 245000
    crit = tp.ICPConvergenceCriteria(max_iteration=50)
    batch = tp.registration_icp_batch(srcs, dsts, rs, inits, crit)
    for k in range(len(srcs)):
        alone = tp.registration_icp(srcs[k], dsts[k], rs[k], inits[k], criteria=crit)
        assert same_bits(batch[k], alone), k
    assert batch[64].fitness == 0 and batch[65].fitness == 0 and batch[66].fitness == 0
    assert len(batch[66].correspondence_set) == 0 and batch[66].iterations == 1
    assert batch[-1].fitness > 0.5 and batch[-1].iterations >= 1


def test_same_call_twice_gives_the_same_bits():
    srcs, dsts, rs, inits = mixed_batch()
    a = tp.registration_icp_batch(srcs, dsts, rs, inits)
    b = tp.registration_icp_batch(srcs, dsts, rs, inits)
    assert all(same_bits(x, y) for x, y in zip(a, b))


def test_far_from_the_origin():
    """The config-5 pair and its seed moved by s = (1e5, -2e5, 3e4) m.  A stored coordinate there carries ~3e-11 m of
    rounding, so ANY implementation's rotation is good to ~1e-12 only, and in the shifted frame T's translation column
    (s - R s + t) carries that rotation noise times the 2e5 m lever arm: the restatement's own shifted and un-shifted
    runs differ by 2.8e-7 m there.  The issue's ||dT||_F < 1e-9 bar therefore cannot hold in the shifted frame for any
    pair of implementations (measured GPU vs restatement: 9.0e-7, all of it dR x s).  The bars below compare the
    rotation, and the translation expressed in the un-shifted frame (un T sh, which removes the lever arm), at about
    ten times the measured differences:
      GPU vs restatement (shifted input)   ||dR||_F 5.8e-12, dt 6.8e-10 m (the restatement's own), rmse 2.4e-11 rel
      GPU shifted vs GPU un-shifted         max|dR| 3.6e-12, dt 3.6e-11 m
    Uncentred sums (sum p q^T - n mu mu^T with |p| ~ 2e5 m: 4e10 m^2 against a 1e-3 m^2 signal) would miss these by
    many orders of magnitude."""
    P, Q, r, init = R.config5_problem()
    s = np.array([1e5, -2e5, 3e4])
    shift = np.eye(4)
    shift[:3, 3] = s
    unshift = np.eye(4)
    unshift[:3, 3] = -s
    crit = tp.ICPConvergenceCriteria(max_iteration=100)
    init_far = shift @ init @ unshift  # the same pose expressed for both clouds moved by s
    ref = R.registration_icp(P + s, Q + s, r, init_far, max_iteration=100)
    gpu = tp.registration_icp(P + s, Q + s, r, init_far, criteria=crit)
    assert gpu.iterations == ref["iterations"]
    assert np.array_equal(gpu.correspondence_set, ref["correspondence_set"])
    assert gpu.fitness == ref["fitness"]
    assert abs(gpu.inlier_rmse - ref["inlier_rmse"]) <= 3e-10 * ref["inlier_rmse"]
    assert np.linalg.norm(gpu.transformation[:3, :3] - ref["transformation"][:3, :3]) < 6e-11
    back, ref_back = unshift @ gpu.transformation @ shift, unshift @ ref["transformation"] @ shift
    assert np.abs(back[:3, 3] - ref_back[:3, 3]).max() < 1e-8
    near = tp.registration_icp(P, Q, r, init, criteria=crit)
    assert np.array_equal(gpu.correspondence_set, near.correspondence_set)
    assert np.abs(back[:3, :3] - near.transformation[:3, :3]).max() < 4e-11
    assert np.abs(back[:3, 3] - near.transformation[:3, 3]).max() < 4e-10


def solve_c(P, Q, r, max_iteration=0):
    """teaser_hip_icp_solve directly (identity init): (result record, correspondence pairs)."""
    L = tp.lib()
    h, lock = tp.icp._handle(-1)
    P, Q = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    corr = np.zeros((max(len(P), 1), 2), dtype=np.int32)
    p = tp.icp.IcpParamsC(r, max_iteration, 1e-6, 1e-6)
    out = tp.icp.IcpResultC()
    dp = C.POINTER(C.c_double)
    with lock:
        rc = L.teaser_hip_icp_solve(h, P.ctypes.data_as(dp), len(P), Q.ctypes.data_as(dp), len(Q), None, C.byref(p),
                                    C.byref(out), corr.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0
    return out, corr[:out.n_correspondences]


def test_ties_and_the_radius_boundary_on_the_gpu():
    """Every source point of a lattice has six targets at exactly the same distance 0.25 (indices shuffled, so the
    smallest index is anywhere in the bucket order the fill's atomics produce): the match must be the smallest index.
    Further sources have their only target at exactly r = 0.5 on an axis: no match (strict d2 < r r)."""
    g = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    offs = np.array([[0.25, 0, 0], [-0.25, 0, 0], [0, 0.25, 0], [0, -0.25, 0], [0, 0, 0.25], [0, 0, -0.25]])
    tgt = (g[:, None, :] + offs[None]).reshape(-1, 3)
    perm = np.random.default_rng(3).permutation(len(tgt))
    Q = np.empty_like(tgt)
    Q[perm] = tgt  # target k of source i, offset o, now has index perm[6 i + o]
    far = np.array([[20.0 + 2 * k, 0.0, 0.0] for k in range(10)])
    Qb = far + np.array([0.5, 0.0, 0.0])
    P = np.concatenate([g, far])
    Q = np.concatenate([Q, Qb])
    out, corr = solve_c(P, Q, 0.5)
    expect = perm.reshape(-1, 6).min(axis=1)
    assert out.n_correspondences == len(g) and out.iterations == 0
    assert np.array_equal(corr[:, 0], np.arange(len(g))) and np.array_equal(corr[:, 1], expect)
    assert out.fitness == len(g) / len(P) and out.inlier_rmse == 0.25
    j, _, fit, rmse = R.corr(P, Q, 0.5)
    assert np.array_equal(j[: len(g)], expect) and (j[len(g):] == -1).all()
    # just inside the boundary the far sources match
    out2, corr2 = solve_c(P, Q, np.nextafter(0.5, 1.0))
    assert out2.n_correspondences == len(P) and np.array_equal(corr2[len(g):, 1], len(tgt) + np.arange(10))


def test_large_radius_degrades_to_brute_force():
    """r = 50 against a unit-cube cloud: every target is a candidate of every source (one grid cell)."""
    rng = np.random.default_rng(17)
    P = rng.uniform(0, 1, size=(600, 3))
    Q = R.apply(pose([1, 1, 0], 3.0, [0.02, 0.0, -0.01]), P) + rng.normal(0, 0.002, size=(600, 3))
    ref = R.registration_icp(P, Q, 50.0, np.eye(4))
    gpu = tp.registration_icp(P, Q, 50.0, np.eye(4))
    assert ref["fitness"] == 1.0
    assert_matches(gpu, ref)


def test_threads_share_the_handle_safely():
    """Python threads calling registration_icp at once (one shared handle per device) get the results of
    sequential calls, bit for bit."""
    import threading
    P, Q, r, init = R.config5_problem()
    rng = np.random.default_rng(9)
    inits = [pose(rng.normal(size=3), rng.uniform(0, 3), rng.normal(0, 0.02, 3)) @ init for _ in range(8)]
    seq = [tp.registration_icp(P, Q, r, T) for T in inits]
    par = [None] * len(inits)

    def work(k):
        par[k] = tp.registration_icp(P, Q, r, inits[k])

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(inits))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(same_bits(a, b) for a, b in zip(seq, par))


def test_invalid_arguments_are_refused():
    L = tp.lib()
    h, lock = tp.icp._handle(-1)
    P = np.ascontiguousarray(np.random.default_rng(0).uniform(size=(10, 3)))
    dp = C.POINTER(C.c_double)

    def run(src=P, dst=P, n_s=10, n_t=10, r=0.1, it=30, rf=1e-6, rr=1e-6, init=None):
        p = tp.icp.IcpParamsC(r, it, rf, rr)
        out = tp.icp.IcpResultC()
        sp = None if src is None else src.ctypes.data_as(dp)
        tq = None if dst is None else dst.ctypes.data_as(dp)
        ip = None if init is None else np.ascontiguousarray(init, dtype=np.float64).ctypes.data_as(dp)
        with lock:
            rc = L.teaser_hip_icp_solve(h, sp, n_s, tq, n_t, ip, C.byref(p), C.byref(out), None)
            return rc, L.teaser_hip_icp_last_error(h).decode()

    assert run()[0] == 0
    bad_last = np.eye(4)
    bad_last[3, 0] = 1e-3
    nan_init = np.eye(4)
    nan_init[0, 3] = np.nan
    nan_pts = P.copy()
    nan_pts[3, 1] = np.inf
    cases = [(dict(r=0.0), "max_correspondence_distance"), (dict(r=-1.0), "max_correspondence_distance"),
             (dict(r=float("nan")), "max_correspondence_distance"),
             (dict(r=float("inf")), "max_correspondence_distance"),
             (dict(it=-1), "max_iteration"), (dict(rf=-1e-6), "relative_fitness"), (dict(rr=-1.0), "relative_rmse"),
             (dict(init=bad_last), "init"), (dict(init=nan_init), "init"), (dict(src=nan_pts), "src"),
             (dict(dst=nan_pts), "dst"), (dict(src=None), "src"), (dict(dst=None), "dst")]
    for kw, name in cases:
        rc, msg = run(**kw)
        assert rc == 1 and name in msg, (kw, rc, msg)
    assert run(src=None, n_s=0)[0] == 0 and run(dst=None, n_t=0)[0] == 0
    with pytest.raises(tp.TeaserHipError, match="BAD_ARG"):
        tp.registration_icp(P, P, 0.1, bad_last)


def test_cxx_facade_reproduces_python():
    from icp_cxx import build_icp_example
    exe = build_icp_example()
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 0
    P, Q, r, init = R.config5_problem()
    py = tp.registration_icp(P, Q, r, init, criteria=tp.ICPConvergenceCriteria(max_iteration=100))
    with tempfile.TemporaryDirectory() as d:
        P.tofile(os.path.join(d, "src.bin"))
        Q.tofile(os.path.join(d, "dst.bin"))
        init.tofile(os.path.join(d, "init.bin"))
        out = subprocess.run([exe, d, repr(r), "100"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    vals = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()}
    assert np.array_equal(np.array([float(v) for v in vals["T"]]).reshape(4, 4), py.transformation)
    assert float(vals["fitness"][0]) == py.fitness and float(vals["rmse"][0]) == py.inlier_rmse
    assert int(vals["iterations"][0]) == py.iterations
    assert int(vals["correspondences"][0]) == len(py.correspondence_set)


def test_example_script_refines():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "teaser_python_fpfh.py"), "--icp"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("ICP ")]
    before = float(next(ln for ln in lines if "before" in ln).split("fitness")[1].split()[0])
    after = float(next(ln for ln in lines if "after" in ln).split("fitness")[1].split()[0])
    assert after >= before
