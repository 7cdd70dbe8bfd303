"""The numpy restatement of pose-graph optimisation (tests/posegraph_reference.py) on its own: it solves what it is
meant to solve, its pieces are consistent with each other, and the two scenarios a device implementation is to be
compared on leave the restatement's own decisions room (gain ratios away from 0, stop tests away from their
thresholds).  No GPU; the library has no pose-graph optimiser yet."""
import numpy as np
import pytest

import posegraph_reference as G


def rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose(axis, deg, t):
    T = np.eye(4)
    T[:3, :3] = rot(axis, deg)
    T[:3, 3] = t
    return T


CHORDS = ((0, 3), (1, 5), (2, 6))
PERTURBATION = dict(angle=0.02, shift=0.02)  # radians / metres, the scale of the start's error per node


def ring(seed=1, n=7, gross=None):
    """True poses on a circle, the ring edges i+1 -> i (certain) and three chords (uncertain), information = I, all
    consistent; the start is the truth perturbed per node (node 0, the reference, is not).  gross: the chord whose
    measurement is replaced by one that is 30 degrees and 1 m off."""
    rng = np.random.default_rng(seed)
    truth = np.stack([pose([0.2, 0.3, 1.0], 360.0 * i / n, [np.cos(2 * np.pi * i / n), np.sin(2 * np.pi * i / n), 0.1 * i])
                      for i in range(n)])
    edges = []
    for i in range(n):
        s, t = (i + 1) % n, i
        edges.append((s, t, G.inverse(truth[t]) @ truth[s], np.eye(6), False))
    for k, (a, b) in enumerate(CHORDS):
        X = G.inverse(truth[a]) @ truth[b]
        if gross == k:
            X = X @ pose([1.0, -0.5, 0.3], 30.0, [0.6, -0.64, 0.48])  # |t| = 1
        edges.append((b, a, X, np.eye(6), True))
    start = truth.copy()
    for i in range(1, n):
        xi = np.concatenate([rng.normal(0, PERTURBATION["angle"], 3), rng.normal(0, PERTURBATION["shift"], 3)])
        start[i] = G.V(xi) @ truth[i]
    return truth, start, edges


def pose_error(a, b):
    return max(np.abs(G.v6(G.inverse(x) @ y)).max() for x, y in zip(a, b))


# F < min_residual with information = I bounds every edge residual by sqrt(min_residual); a node is at most three ring
# edges from the reference, and each entry of an edge's 6-vector is bounded by its norm
POSE_BOUND = 3 * np.sqrt(G.DEFAULTS["min_residual"])


@pytest.mark.parametrize("dtype", (np.float64, np.longdouble))
def test_consistent_ring_is_solved_from_a_perturbed_start(dtype):
    truth, start, edges = ring()
    out = G.global_optimization(start, edges, dtype=dtype)
    assert out["F0"] > 1e-3 and out["F"] < G.DEFAULTS["min_residual"] and out["status"] == G.RESIDUAL
    assert not out["pruned"].any() and out["iterations"][1] == 0
    assert np.array_equal(out["poses"][0], truth[0].astype(dtype))
    err = pose_error(truth, out["poses"].astype(np.float64))
    print("consistent ring (%s): F0 %.3g F %.3g iterations %s pose error %.3g" % (
        dtype.__name__, float(out["F0"]), float(out["F"]), out["iterations"], err))
    assert err < POSE_BOUND


def test_gross_chord_is_pruned_and_the_result_is_the_graph_without_it():
    truth, start, edges = ring(gross=1)
    out = G.global_optimization(start, edges)
    bad = 7 + 1
    assert out["pruned"].tolist() == [k == bad for k in range(len(edges))]
    assert out["confidence"][bad] < G.DEFAULTS["edge_prune_threshold"]
    assert (np.delete(out["confidence"], bad) >= G.DEFAULTS["edge_prune_threshold"]).all()
    assert all(out["confidence"][k] == 1.0 for k in range(7))  # certain edges
    without = G.global_optimization(start, edges[:bad] + edges[bad + 1:])
    assert not without["pruned"].any() and without["F"] < G.DEFAULTS["min_residual"]
    assert out["F"] < G.DEFAULTS["min_residual"]
    print("gross chord: confidence %.3g, iterations %s, against the graph without it %.3g, against the truth %.3g" % (
        out["confidence"][bad], out["iterations"], pose_error(out["poses"], without["poses"]),
        pose_error(out["poses"], truth)))
    assert pose_error(out["poses"], without["poses"]) < 2 * POSE_BOUND and pose_error(out["poses"], truth) < POSE_BOUND


def test_single_pass_when_the_threshold_is_zero_and_trivial_graphs():
    truth, start, edges = ring(gross=1)
    out = G.global_optimization(start, edges, dict(edge_prune_threshold=0.0))
    assert not out["pruned"].any() and len(out["passes"]) == 1 and out["confidence"][8] < 0.25
    one = G.global_optimization(start[:1], [])
    assert one["status"] == G.TRIVIAL and np.array_equal(one["poses"], start[:1])
    none = G.global_optimization(start, [])
    assert none["status"] == G.TRIVIAL and np.array_equal(none["poses"], start)


def test_v_and_v6_round_trip_in_both_branches():
    rng = np.random.default_rng(2)
    for _ in range(50):
        xi = np.concatenate([rng.uniform(-3, 3, 1), rng.uniform(-1.5, 1.5, 1), rng.uniform(-3, 3, 1), rng.normal(0, 2, 3)])
        assert np.allclose(G.v6(G.V(xi)), xi, rtol=0, atol=1e-12)
    for b in (np.pi / 2, -np.pi / 2):  # sy <= 1e-6: gamma is reported as 0 and alpha carries the rotation that is left
        xi = np.array([0.7, b, -0.4, 1.0, 2.0, 3.0])
        M = G.V(xi)
        assert np.sqrt(M[0, 0] ** 2 + M[1, 0] ** 2) <= 1e-6
        back = G.v6(M)
        assert back[2] == 0.0 and abs(back[1] - b) < 1e-7
        assert np.allclose(G.V(back), M, rtol=0, atol=1e-7)
    assert np.array_equal(G.V(np.zeros(6)), np.eye(4)) and np.array_equal(G.v6(np.eye(4)), np.zeros(6))
    for c, D in enumerate(G.generators()):  # the generators are the derivatives of V at 0
        h = np.zeros(6)
        h[c] = 1e-6
        assert np.allclose((G.V(h) - G.V(-h)) / 2e-6, D, rtol=0, atol=1e-9)


def test_jacobian_is_the_derivative_of_the_residual_on_a_consistent_graph():
    """lin6 is the derivative of v6 at the identity, so J is the derivative of e_k exactly where e_k = 0."""
    truth, _, edges = ring()
    h = 1e-6
    for E in (edges[0], edges[3], edges[8]):
        s, t = E[0], E[1]
        J = G.jacobian(truth, E)
        for node, sign in ((s, 1.0), (t, -1.0)):
            fd = np.zeros((6, 6))
            for c in range(6):
                d = np.zeros(6)
                d[c] = h
                up, dn = truth.copy(), truth.copy()
                up[node], dn[node] = G.V(d) @ truth[node], G.V(-d) @ truth[node]
                fd[:, c] = (G.residuals(up, [E], 0.0)[0][0] - G.residuals(dn, [E], 0.0)[0][0]) / (2 * h)
            assert np.allclose(fd, sign * J, rtol=0, atol=1e-8)


def test_linearisation_is_consistent_with_the_objective():
    """g is half the gradient of F for fixed weights where J is exact, H is symmetric with zero reference rows, and
    the first step reduces F."""
    truth, start, edges = ring()
    lin = G.linearize(start, edges)
    assert np.allclose(lin["H"], lin["H"].T, rtol=0, atol=1e-12) and not lin["H"][:6].any() and not lin["g"][:6].any()
    assert lin["mu"] == pytest.approx(0.03 ** 2) and (lin["l"][:7] == 1).all() and (lin["l"][7:] < 1).all()
    step = G.first_step(start, edges)
    cand = np.stack([G.V(step["d"][6 * i:6 * i + 6]) @ start[i] for i in range(len(start))])
    assert G.residuals(cand, edges, lin["mu"])[3] < lin["F"]
    # the float64 solve against the longdouble one: the backward error of an N x N Cholesky solve and of the sums
    # that build H and g is a small multiple of N eps, amplified by the condition number of H + lam I
    wide = G.first_step(start, edges, dtype=np.longdouble)
    N = len(step["A"])
    bound = N * np.finfo(np.float64).eps * np.linalg.cond(step["A"]) * np.linalg.norm(step["d"])
    err = np.abs(wide["d"].astype(np.float64) - step["d"]).max()
    print("first step: float64 against longdouble %.3g, bound %.3g" % (err, bound))
    assert err <= bound


@pytest.mark.parametrize("gross", (None, 1))
def test_scenarios_leave_the_decisions_room(gross):
    """What a comparison of accept / reject sequences, iteration counts, pruned sets and stop reasons against this
    restatement presupposes: in the reference run every gain ratio is at least 1e-3 away from 0 and every stop test
    that does not fire is a factor 2 away from its threshold.  Perturbation used: PERTURBATION, seed 1."""
    _, start, edges = ring(gross=gross)
    out = G.global_optimization(start, edges)
    for p in out["passes"]:
        for row in p["trace"]:
            if row["kind"] == "trial":
                assert row["rho"] is not None and abs(row["rho"]) >= 1e-3, row
            elif not row["fires"]:
                ratio = row["value"] / row["threshold"]
                assert ratio >= 2 or ratio <= 0.5, row
