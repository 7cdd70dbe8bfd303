"""Information matrices on the MI355X (include/teaser_hip.h, "Information matrices") against the numpy restatement
(tests/information_reference.py): bit-equal where every product and sum is exact (integer grids under a signed axis
permutation and an integer shift), inside the bound of a sum of |C| terms taken in any order on the bunny,
|L - L_ref| <= (|C| + 3) 2^-52 SUM_j |term_j| elementwise (L_ref and the right-hand side from the restatement, in
np.longdouble where that is wider than double); the correspondences of registration_icp(max_iteration=0, init=T); the
same bits alone and anywhere in a mixed batch.  Source sizes: 0, 1, kIcpBlock - 1, kIcpBlock, kIcpBlock + 1 and three
blocks; target sizes 0 and 1."""
import ctypes as C
import importlib

import numpy as np
import pytest

import icp_reference as R
import information_reference as I
from information_reference import grid_pair
from util import golden

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")

K_ICP_BLOCK = 256
SIZES = (0, 1, K_ICP_BLOCK - 1, K_ICP_BLOCK, K_ICP_BLOCK + 1, 2 * K_ICP_BLOCK + 188)
WIDE = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def bunny():
    b = np.asarray(golden()["bunny"], dtype=np.float64)
    return np.ascontiguousarray(b.T if b.shape[0] == 3 else b)


def rigid(seed, t_scale):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = rng.normal(size=3) * t_scale
    return T


@pytest.fixture(scope="module")
def bunny_pair():
    """The bunny moved by a random rigid T (the target is T applied to a noisy copy, so most points match within r)."""
    B = bunny()
    T = rigid(17, 0.2)
    rng = np.random.default_rng(18)
    Q = R.apply(T, B + rng.normal(0, 0.0005, size=B.shape))[rng.permutation(len(B))[: len(B) - 200]]
    return B, np.ascontiguousarray(Q), T, 0.004


def info_batch(Ps, Qs, rs, Ts):
    return tp.get_information_matrix_from_point_clouds_batch(Ps, Qs, rs, Ts, return_results=True)


@pytest.mark.parametrize("n_s", SIZES)
def test_integer_grid_is_bit_equal_to_numpy(n_s):
    P, Q, T = grid_pair(100 + n_s, n_s, 300)
    ref = I.information(P, Q, 0.5, T)
    info, res = info_batch([P], [Q], 0.5, T)
    assert len(ref["correspondence_set"]) == (2 * n_s + 2) // 3
    assert np.array_equal(res[0].correspondence_set, ref["correspondence_set"])
    assert info[0].tobytes() == (ref["information"] + 0.0).tobytes()
    assert info[0][5, 5] == len(ref["correspondence_set"])


@pytest.mark.parametrize("n_t", (0, 1))
def test_tiny_targets(n_t):
    for n_s in SIZES:
        P, Q, T = grid_pair(7 + n_s, n_s, n_t)
        ref = I.information(P, Q, 0.5, T)
        info, res = info_batch([P], [Q], 0.5, T)
        assert info[0].tobytes() == (ref["information"] + 0.0).tobytes()
        assert res[0].fitness == ref["fitness"] and len(res[0].correspondence_set) == len(ref["correspondence_set"])
        if n_t == 0:
            assert not info[0].any() and res[0].fitness == 0.0


def test_bunny_within_the_bound_of_a_sum_in_any_order(bunny_pair):
    P, Q, T, r = bunny_pair
    info, res = info_batch([P], [Q], r, T)
    icp = tp.registration_icp(P, Q, r, T, criteria=tp.ICPConvergenceCriteria(max_iteration=0))
    cs = res[0].correspondence_set
    n = len(cs)
    assert n > 1000 and n < len(P)
    assert np.array_equal(cs, icp.correspondence_set) and np.array_equal(cs, R.registration_icp(P, Q, r, T, 0)["correspondence_set"])
    assert res[0].fitness == icp.fitness and res[0].inlier_rmse == icp.inlier_rmse and res[0].iterations == 0
    assert res[0].transformation.tobytes() == T.tobytes()
    ref, mag = I.information_vectorised(Q, cs[:, 1], dtype=WIDE)
    err = np.abs(info[0].astype(WIDE) - ref)
    bound = (n + 3) * WIDE(2.0) ** -52 * mag
    print("information, bunny: |C| = %d, largest error / bound = %.3g" % (n, float((err / np.maximum(bound, WIDE(1e-300))).max())))
    assert (err <= bound).all()
    assert info[0][5, 5] == n and np.array_equal(info[0][3:, 3:], n * np.eye(3))
    assert np.array_equal(info[0], info[0].T)


def test_no_point_within_r_gives_the_zero_matrix(bunny_pair):
    P, Q, T, r = bunny_pair
    far = T.copy()
    far[:3, 3] += 10.0
    info, res = info_batch([P], [Q], r, far)
    assert not info[0].any() and res[0].fitness == 0.0 and res[0].inlier_rmse == 0.0
    assert len(res[0].correspondence_set) == 0


def test_evaluate_registration_is_the_zero_iteration_icp(bunny_pair):
    P, Q, T, r = bunny_pair
    a = tp.evaluate_registration(P, Q, r, T)
    b = tp.registration_icp(P, Q, r, T, criteria=tp.ICPConvergenceCriteria(max_iteration=0))
    assert a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse and a.iterations == 0
    assert np.array_equal(a.correspondence_set, b.correspondence_set) and a.transformation.tobytes() == T.tobytes()
    e = tp.evaluate_registration(P, P, r)
    assert e.fitness == 1.0 and e.inlier_rmse == 0.0 and np.array_equal(e.transformation, np.eye(4))
    both = tp.evaluate_registration_batch([P, P], [Q, P], r, [T, np.eye(4)])
    assert both[0].fitness == a.fitness and both[1].fitness == 1.0


def test_same_bits_alone_and_anywhere_in_a_mixed_batch(bunny_pair):
    P, Q, T, r = bunny_pair
    others = [grid_pair(40 + n, n, 300) for n in SIZES]
    alone, alone_res = info_batch([P], [Q], r, T)
    again, _ = info_batch([P], [Q], r, T)
    assert alone.tobytes() == again.tobytes()
    singles = [info_batch([p], [q], 0.5, t)[0][0] for p, q, t in others]
    for at in (0, 3, len(others)):
        Ps = [o[0] for o in others]
        Qs = [o[1] for o in others]
        Ts = [o[2] for o in others]
        rs = [0.5] * len(others)
        Ps.insert(at, P), Qs.insert(at, Q), Ts.insert(at, T), rs.insert(at, r)
        info, res = info_batch(Ps, Qs, rs, np.stack(Ts))
        assert info[at].tobytes() == alone[0].tobytes()
        assert np.array_equal(res[at].correspondence_set, alone_res[0].correspondence_set)
        assert res[at].fitness == alone_res[0].fitness and res[at].inlier_rmse == alone_res[0].inlier_rmse
        rest = [k for k in range(len(Ps)) if k != at]
        for k, single in zip(rest, singles):
            assert info[k].tobytes() == single.tobytes()
    assert not singles[0].any()  # the empty problem of the batch


def test_c_entry_one_problem_form_and_refusals(bunny_pair):
    P, Q, T, r = bunny_pair
    one = tp.get_information_matrix_from_point_clouds(P, Q, r, T)
    assert one.tobytes() == info_batch([P], [Q], r, T)[0][0].tobytes()
    L = tp.lib()
    from importlib import import_module
    icp = import_module("teaser-plusplus_amd.icp")
    h = icp._handle(-1)
    dp = C.POINTER(C.c_double)
    info = np.full(36, -3.0)
    with h.lock:
        rc = L.teaser_hip_icp_information(h.h, P.ctypes.data_as(dp), len(P), Q.ctypes.data_as(dp), len(Q),
                                          T.ctypes.data_as(dp), r, info.ctypes.data_as(dp), None, None)
    assert rc == 0 and info.tobytes() == one.tobytes()
    bad = T.copy()
    bad[3, 3] = 2.0
    with pytest.raises(tp.TeaserHipError, match="last row"):
        tp.get_information_matrix_from_point_clouds(P, Q, r, bad)
    with pytest.raises(tp.TeaserHipError, match="max_correspondence_distance"):
        tp.get_information_matrix_from_point_clouds(P, Q, 0.0, T)
    bad = T.copy()
    bad[0, 3] = np.nan
    with pytest.raises(tp.TeaserHipError, match="transformation"):
        tp.get_information_matrix_from_point_clouds(P, Q, r, bad)
    assert tp.get_information_matrix_from_point_clouds(P, Q, r, T).tobytes() == one.tobytes()  # still serves


def test_cxx_facade_reproduces_python(bunny_pair):
    import os
    import subprocess
    import tempfile

    from information_cxx import build_information_example
    exe = build_information_example()
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 0
    P, Q, T, r = bunny_pair
    info, res = info_batch([P], [Q], r, T)
    with tempfile.TemporaryDirectory() as d:
        P.tofile(os.path.join(d, "src.bin"))
        Q.tofile(os.path.join(d, "dst.bin"))
        T.tofile(os.path.join(d, "T.bin"))
        out = subprocess.run([exe, d, repr(r)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    vals = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()}
    assert np.array([float(v) for v in vals["information"]]).reshape(6, 6).tobytes() == info[0].tobytes()
    assert float(vals["fitness"][0]) == res[0].fitness and float(vals["rmse"][0]) == res[0].inlier_rmse
    assert int(vals["correspondences"][0]) == len(res[0].correspondence_set)
