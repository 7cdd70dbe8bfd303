"""The Colored-ICP contract (include/teaser_hip.h, "ICP refinement: Colored ICP") as restated in numpy
(tests/icp_colored_reference.py) against closed forms and against the point-to-plane restatement, the decision margins
of the textured scene the GPU tests use, and the surface of the GPU implementation that needs no device: names,
defaults, ValueErrors, exported symbols, struct sizes, which entry point a call reaches."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import icp_colored_reference as RC
import icp_plane_reference as RP
from icp_colored_cases import KERNEL_CASES, scene, scene_gradients
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")


@pytest.fixture(scope="module", autouse=True)
def _the_library_declares_what_is_restated():
    """The restatement restates a contract of the library: without its entry points none of this stands."""
    assert "teaser_hip_icp_batch_color" in tp.EXPORTED_SYMBOLS and hasattr(tp, "registration_colored_icp")


def run(kernel="l2", k=1.0, **kw):
    s = scene()
    kw.setdefault("max_iteration", 50)
    return RC.registration_icp(s["source"], s["target"], s["source_colors"], s["target_colors"], s["target_normals"],
                               s["r"], kernel=kernel, k=k, gradients=scene_gradients(0, 30), **kw)


# ---- the surface that needs no device ------------------------------------------------------------------------------
def test_public_names_defaults_and_value_errors():
    for name in ("TransformationEstimationForColoredICP", "registration_colored_icp", "estimate_color_gradients",
                 "estimate_color_gradients_batch"):
        assert name in tp.__all__ and hasattr(tp, name), name
    e = tp.TransformationEstimationForColoredICP()
    assert e.lambda_geometric == 0.968 and isinstance(e.kernel, tp.L2Loss) and e.gradient_max_nn == 30
    assert list(inspect.signature(tp.TransformationEstimationForColoredICP).parameters)[:2] == ["lambda_geometric",
                                                                                                 "kernel"]
    sig = inspect.signature(tp.registration_colored_icp).parameters
    assert list(sig)[:6] == ["source", "target", "max_correspondence_distance", "init", "estimation_method", "criteria"]
    for name in ("source_colors", "target_colors", "target_normals", "gradient_radius", "gradient_max_nn",
                 "target_color_gradients", "device"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert sig["gradient_radius"].default is None and sig["gradient_max_nn"].default == 30
    assert sig["device"].default == -1
    assert inspect.signature(tp.estimate_color_gradients).parameters["max_nn"].default == 30
    for fn in (tp.registration_icp, tp.registration_icp_batch):
        p = inspect.signature(fn).parameters
        for name in ("source_colors", "target_colors", "target_color_gradients"):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is None
    assert list(inspect.signature(tp.registration_icp).parameters)[:7] == [
        "source", "target", "max_correspondence_distance", "init", "estimation_method", "criteria", "device"]
    assert list(inspect.signature(tp.registration_icp_batch).parameters)[:10] == [
        "sources", "targets", "max_correspondence_distance", "inits", "criteria", "device", "estimation_methods",
        "target_normals", "source_covariances", "target_covariances"]
    r = tp.icp.IcpColorC(7.0, 7.0, 7, 7)
    L = tp.lib()
    assert L.teaser_hip_icp_color_default(r) == 0
    assert (r.lambda_geometric, r.gradient_radius, r.gradient_max_nn, r.reserved) == (0.968, 0.0, 30, 0)
    assert L.teaser_hip_icp_color_default(None) == 1
    for bad in (dict(lambda_geometric=-0.1), dict(lambda_geometric=1.5), dict(lambda_geometric=float("nan")),
                dict(kernel="tukey"), dict(gradient_max_nn=3), dict(gradient_max_nn=101), dict(gradient_radius=0.0),
                dict(gradient_radius=float("inf"))):
        with pytest.raises(ValueError):
            tp.TransformationEstimationForColoredICP(**bad)
    # refused before any library call (no device is needed to get these)
    P = np.zeros((5, 3))
    est = tp.TransformationEstimationForColoredICP()
    full = dict(source_colors=P, target_colors=P, target_normals=P)
    for missing in full:
        kw = {k: v for k, v in full.items() if k != missing}
        with pytest.raises(ValueError, match=missing):
            tp.registration_colored_icp(P, P, 0.1, **kw)
        with pytest.raises(ValueError, match=missing):
            tp.registration_icp(P, P, 0.1, np.eye(4), est, **kw)
    with pytest.raises(ValueError, match="source_colors"):
        tp.registration_icp_batch([P, P], [P, P], 0.1, estimation_methods=[None, est], target_normals=[None, P],
                                  source_colors=[None, None], target_colors=[None, P])
    with pytest.raises(ValueError, match="target_normals"):
        tp.registration_icp_batch([P], [P], 0.1, estimation_methods=[est], source_colors=[P], target_colors=[P],
                                  target_normals=[tp.KDTreeSearchParamKNN(10)])
    with pytest.raises(ValueError, match="shape"):
        tp.registration_colored_icp(P, P, 0.1, **dict(full, target_colors=np.zeros((4, 3))))
    with pytest.raises(ValueError):
        tp.registration_colored_icp(P, P, 0.1, np.eye(4), tp.TransformationEstimationPointToPlane(), **full)
    with pytest.raises(ValueError, match="max_nn"):
        tp.estimate_color_gradients(P, P, P, 0.1, max_nn=3)
    with pytest.raises(ValueError, match="radius"):
        tp.estimate_color_gradients(P, P, P, -1.0)


def test_header_declares_and_library_exports_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "teaser_hip.h")).read()
    L = tp.lib()
    counts = {"teaser_hip_icp_color_default": 1, "teaser_hip_icp_batch_color": 18, "teaser_hip_icp_solve_color": 17,
              "teaser_hip_icp_color_gradients_batch": 9}
    for name, argc in counts.items():
        assert re.search(r"TEASER_HIP_API int32_t %s\(" % name, text), name
        assert name in tp.EXPORTED_SYMBOLS and len(getattr(L, name).argtypes) == argc, name
    assert "typedef struct teaser_icp_color_c" in text and "sizeof(teaser_icp_color_c) == 24" in text
    assert C.sizeof(tp.icp.IcpColorC) == 24
    assert C.sizeof(tp.icp.IcpEstimationC) == 16 and C.sizeof(tp.icp.IcpNormalSearchC) == 48  # layouts unchanged
    assert C.sizeof(tp.icp.IcpParamsC) == 32 and C.sizeof(tp.icp.IcpResultC) == 152
    assert L.teaser_hip_abi_version() == 1
    # a NULL handle answers BAD_ARG
    assert L.teaser_hip_icp_batch_color(None, 0, *([None] * 16)) == 1
    assert L.teaser_hip_icp_solve_color(None, None, 0, None, 0, *([None] * 12)) == 1
    assert L.teaser_hip_icp_color_gradients_batch(None, 0, *([None] * 7)) == 1


def test_only_calls_with_a_coloured_problem_reach_the_color_entry(monkeypatch):
    calls = []

    class FakeLib:
        def teaser_hip_icp_create(self, device, out):
            out._obj.value = 4096
            return 0

        def teaser_hip_icp_last_error(self, h):
            return b""

        def teaser_hip_icp_destroy(self, h):
            return 0

    for name in ("batch", "batch_ex", "batch_cov", "batch_auto", "batch_color"):
        setattr(FakeLib, "teaser_hip_icp_" + name,
                lambda self, *a, _n=name: calls.append((_n, len(a))) or 0)
    monkeypatch.setattr(tp, "lib", lambda: FakeLib())
    monkeypatch.setattr(tp.icp._cache, "handles", {})
    monkeypatch.setattr(tp._handles, "_current_device", lambda: 0)
    P = np.zeros((4, 3))
    cov = np.tile(np.eye(3), (4, 1, 1))
    plane = tp.TransformationEstimationPointToPlane()
    tp.registration_icp(P, P, 0.1)
    tp.registration_icp(P, P, 0.1, np.eye(4), plane, target_normals=P)
    tp.registration_icp(P, P, 0.1, np.eye(4), tp.TransformationEstimationForGeneralizedICP(), source_covariances=cov,
                        target_covariances=cov)
    tp.registration_icp(P, P, 0.1, np.eye(4), plane, target_normals=tp.KDTreeSearchParamKNN(3))
    tp.registration_icp(P, P, 0.1, np.eye(4), plane, target_normals=P, source_colors=P, target_colors=P)  # ignored
    assert calls == [("batch", 10), ("batch_ex", 12), ("batch_cov", 14), ("batch_auto", 15), ("batch_ex", 12)]
    del calls[:]
    tp.registration_colored_icp(P, P, 0.1, source_colors=P, target_colors=P, target_normals=P)
    tp.registration_icp_batch([P, P], [P, P], 0.1,
                              estimation_methods=[tp.TransformationEstimationForColoredICP(), None],
                              target_normals=[P, None], source_colors=[P, None], target_colors=[P, None])
    assert calls == [("batch_color", 18), ("batch_color", 18)]


# ---- the restatement -----------------------------------------------------------------------------------------------
def test_lambda_one_is_the_point_to_plane_restatement():
    s = scene()
    for kernel, k in (("l2", 1.0), ("tukey", 0.01)):
        a = run(kernel, k, lam=1.0)
        b = RP.registration_icp(s["source"], s["target"], s["target_normals"], s["r"], kernel=kernel, k=k,
                                max_iteration=50)
        assert np.array_equal(a["transformation"], b["transformation"]) and a["iterations"] == b["iterations"] >= 2
        assert np.array_equal(a["correspondence_set"], b["correspondence_set"])


def test_gradient_of_a_linear_intensity_on_a_plane_is_its_tangential_part():
    """I = a . p + b on an exact plane with unit normal n: the gradient is a - (a . n) n.  The restatement's largest
    error over the cases below is 4.53e-13 (measured with this file); the bar is 1000 times that."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for case in range(4):
        n = rng.standard_normal(3)
        n /= np.linalg.norm(n)
        u = np.cross(n, [1.0, 0.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        st = rng.uniform(-1, 1, (400, 2))
        P = st[:, :1] * u + st[:, 1:] * v + 0.3 * n
        P = P - ((P - 0.3 * n) @ n)[:, None] * n  # back onto the plane after rounding
        a, b = rng.standard_normal(3), 0.4
        i = P @ a + b
        g, ms, _, _ = RC.color_gradients(P, np.tile(n, (len(P), 1)), np.stack([i, i, i], 1), 0.25, (30, 100)[case % 2],
                                         details=True)
        want = a - (a @ n) * n
        worst = max(worst, float(np.abs(g[ms >= 4] - want).max()))
        assert (ms >= 4).sum() > 300
    print("largest error %.3g" % worst)
    assert worst < 1000 * 4.53e-13


def test_solve3_matches_a_dense_solve_and_refuses_bad_pivots():
    rng = np.random.default_rng(4)
    M = rng.normal(size=(10, 3))
    G, h = M.T @ M, rng.normal(size=3)
    assert np.allclose(RC.solve3(G, h), np.linalg.solve(G, h), rtol=1e-11)
    G0 = G.copy()
    G0[1, :] = G0[:, 1] = 0.0
    assert not RC.solve3(G0, h).any() and not RC.solve3(-G, h).any()
    Gn = G.copy()
    Gn[0, 0] = np.nan
    assert not RC.solve3(Gn, h).any()


def test_scene_has_no_zero_gradient_and_colour_pins_what_geometry_lets_slide():
    s = scene()
    assert len(s["target"]) == 2304 and len(s["source"]) == 1500
    for max_nn in (30, 33):
        assert scene_gradients(0, max_nn).any(axis=1).all()
    assert scene_gradients(0, 30).tobytes() != scene_gradients(0, 33).tobytes()
    for kernel, k in KERNEL_CASES:
        col = run(kernel, k)
        pl = RP.registration_icp(s["source"], s["target"], s["target_normals"], s["r"], kernel=kernel, k=k,
                                 max_iteration=50)
        ec = np.linalg.norm(col["transformation"] - s["T_true"])
        ep = np.linalg.norm(pl["transformation"] - s["T_true"])
        print("%s: coloured %.3g (%d its), point-to-plane %.3g (%d its)" % (kernel, ec, col["iterations"], ep,
                                                                             pl["iterations"]))
        assert ec <= ep / 10 and col["iterations"] >= 2, kernel


def test_scene_decision_margins_make_equal_sets_a_fair_demand():
    """Relative gaps between a source point's best and second-best d2, between any d2 and r r, and the distance of the
    stop rule's comparison from its threshold: all many orders above the 1e-15 a different summation order moves d2."""
    for kernel, k in KERNEL_CASES:
        m = run(kernel, k, margins=True)["margins"]
        print(kernel, m)
        assert m["best_gap"] > 1e-7 and m["radius_gap"] > 1e-7 and m["stop_gap"] > 1e-9, (kernel, m)


def test_summation_order_moves_the_pose_far_less_than_the_bar():
    """T under two shuffled orders and 256-row chunks against ascending order: at most 7.6e-17 here (L2 and the four
    kernels), so the project's 1e-9 bar on ||dT||_F stands (it needs three orders of headroom)."""
    worst = 0.0
    for kernel, k in KERNEL_CASES:
        base = run(kernel, k)
        for kw in (dict(order_seed=1), dict(order_seed=2), dict(chunk=256)):
            o = run(kernel, k, **kw)
            assert o["iterations"] == base["iterations"]
            assert np.array_equal(o["correspondence_set"], base["correspondence_set"])
            worst = max(worst, float(np.linalg.norm(o["transformation"] - base["transformation"])))
    print("largest ||dT||_F %.3g" % worst)
    assert worst <= 1e-12
