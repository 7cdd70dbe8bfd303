"""The Python front-end of Fast Global Registration (teaser-plusplus_amd/fgr.py) on the GPU: the single call, the
batched call and the stage call return the C call's pose, the RegistrationResult is evaluate_registration at that
pose, tuple_test=True is the tuple test followed by the plain call, and the feature-matching form is the matcher
followed by the correspondence form."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import fgr_reference as ref
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(ROOT, "tests", "golden", "fgr_golden.npz"))


def c_call(P, Q, corr, **opt):
    """teaser_hip_fgr_correspondence on a handle of its own."""
    L = tp.lib()
    h = C.c_void_p()
    assert L.teaser_hip_fgr_create(-1, C.byref(h)) == 0
    try:
        p = tp.fgr.FgrParamsC()
        L.teaser_hip_fgr_params_default(p)
        for k, v in opt.items():
            setattr(p, k, v)
        out = tp.fgr.FgrResultC()
        P, Q = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
        corr = np.ascontiguousarray(corr, dtype=np.int32)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        rc = L.teaser_hip_fgr_correspondence(h, P.ctypes.data_as(dp), len(P), Q.ctypes.data_as(dp), len(Q),
                                             corr.ctypes.data_as(ip), len(corr), C.byref(p), C.byref(out))
        assert rc == 0, L.teaser_hip_fgr_last_error(h)
        return np.array(out.transformation[:]).reshape(4, 4), out
    finally:
        L.teaser_hip_fgr_destroy(h)


def test_python_returns_the_c_calls_pose_and_the_evaluation_at_it():
    name = "c255"
    P, Q, corr = G[name + "/P"], G[name + "/Q"], G[name + "/corr"]
    T, rec = c_call(P, Q, corr, use_absolute_scale=1)
    o = tp.FastGlobalRegistrationOption(use_absolute_scale=True, tuple_test=False, maximum_correspondence_distance=0.025)
    res = tp.registration_fgr_based_on_correspondence(P, Q, corr, o)
    assert res.transformation.tobytes() == T.tobytes() and res.iterations == rec.iterations == 64
    assert res.fgr["final_mu"] == rec.final_mu and res.fgr["n_corr"] == len(corr)
    ev = tp.evaluate_registration(P, Q, o.maximum_correspondence_distance, T)
    assert (res.fitness, res.inlier_rmse) == (ev.fitness, ev.inlier_rmse)
    assert np.array_equal(res.correspondence_set, ev.correspondence_set) and len(ev.correspondence_set) > 100
    assert np.abs(T - G[name + "/T_true"]).max() < 1e-2
    both = tp.registration_fgr_based_on_correspondence_batch([P, Q], [Q, P], [corr, corr[:, ::-1]], o)
    assert both[0].transformation.tobytes() == T.tobytes()
    assert np.abs(both[1].transformation @ T - np.eye(4)).max() < 1e-2
    st = tp.fgr_iterations_batch([P], [Q], [corr], 64, o)[0]
    assert st["transformation"].tobytes() == T.tobytes() and st["mu"].shape == (64,) and st["A"].shape == (64, 6, 6)
    assert st["p"].shape == (len(corr), 3) and st["trans"].shape == (64, 4, 4)


def test_tuple_test_with_a_seed_is_the_tuple_test_then_the_plain_call():
    P, Q, corr, T_true = ref.make_case(31, 400, 420, 300, outlier=0.5)
    o = tp.FastGlobalRegistrationOption(tuple_test=True, tuple_scale=0.9, seed=17)
    res = tp.registration_fgr_based_on_correspondence(P, Q, corr, o)
    kept = tp.tuple_test_batch([P], [Q], [corr], 0.9, 17)[0]
    plain = tp.registration_fgr_based_on_correspondence(
        P, Q, kept, tp.FastGlobalRegistrationOption(tuple_test=False))
    assert 10 <= len(kept) < len(corr) and np.array_equal(res.fgr_corres, kept)
    assert res.transformation.tobytes() == plain.transformation.tobytes() and res.fgr["n_corr"] == len(kept)
    assert (res.fitness, res.inlier_rmse) == (plain.fitness, plain.inlier_rmse)
    again = tp.registration_fgr_based_on_correspondence(P, Q, corr, o)
    assert again.transformation.tobytes() == res.transformation.tobytes()


def test_feature_matching_form_is_the_matcher_then_the_correspondence_form():
    rng = np.random.default_rng(5)
    P, Q, corr, _ = ref.make_case(32, 200, 200, 200, outlier=0.2, repeats=False)
    fs = rng.standard_normal((200, 33)).astype(np.float32)
    ft = rng.standard_normal((200, 33)).astype(np.float32)
    ft[corr[:160, 1]] = fs[corr[:160, 0]] + 0.01 * rng.standard_normal((160, 33)).astype(np.float32)
    o = tp.FastGlobalRegistrationOption(tuple_test=False)
    res = tp.registration_fgr_based_on_feature_matching(P, Q, fs, ft, o)
    pairs = tp.feature_matching_correspondences(fs, ft, True, 3)
    want = tp.registration_fgr_based_on_correspondence(P, Q, pairs, o)
    assert len(pairs) >= 160 and np.array_equal(res.fgr_corres, pairs)
    assert res.transformation.tobytes() == want.transformation.tobytes()
