"""The scenarios the pose-graph optimiser is compared on against the numpy restatement (tests/posegraph_reference.py),
the margin conditions a scenario has to meet before a comparison of decisions means anything, and the comparison rule.
tests/test_posegraph_cases.py asserts the margins on the CPU; the emulation and the GPU tests use the same cases.

graph() follows ring() of tests/test_posegraph_reference.py (imported for the two scenarios that file defines, which
are used unchanged).  It draws, in order: the information matrices of the ring edges, those of the chords, then one
perturbation per node, the reference node's included (drawn and discarded).

Sizes of class 6 come from the factorisation's tile constant (kPgTile in csrc/posegraph_device.h, read from the
source): N = 6 (n - 1) on both sides of the tile's first two edges, an exact multiple of it, and n = 128."""
import functools
import os
import re

import numpy as np

import posegraph_reference as G
from test_posegraph_reference import CHORDS, pose, ring
from util import ROOT

WIDE = np.finfo(np.longdouble).eps < 1e-18  # the yardstick is wider than double here


def tile_constant():
    text = open(os.path.join(ROOT, "teaser-plusplus_amd", "csrc", "posegraph_device.h")).read()
    return int(re.search(r"constexpr int kPgTile = (\d+);", text).group(1))


def realistic_information(rng, points):
    """SUM G^T G over `points` points uniform in [-1, 1]^3, G = [-[q]x | I] (the information matrix of a registered
    pair with that many correspondences)."""
    L = np.zeros((6, 6))
    for q in rng.uniform(-1, 1, (points, 3)):
        Gq = np.zeros((3, 6))
        Gq[:, :3] = -np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])
        Gq[:, 3:] = np.eye(3)
        L += Gq.T @ Gq
    return L


def graph(seed, n=7, chords=CHORDS, gross=(), ref=0, angle=0.02, shift=0.02, realistic=False, closed=True):
    """True poses on a circle, ring edges i+1 -> i (certain; closed: also 0 -> n-1) and `chords` (a, b) as uncertain
    edges b -> a; the chords whose index is in `gross` measure 30 degrees and 1 m off.  The start is the truth perturbed
    per node (normal, `angle` radians and `shift` metres) except at node `ref`."""
    rng = np.random.default_rng(seed)
    truth = np.stack([pose([0.2, 0.3, 1.0], 360.0 * i / n, [np.cos(2 * np.pi * i / n), np.sin(2 * np.pi * i / n), 0.1 * i])
                      for i in range(n)])
    n_ring = n if closed else n - 1
    info_ring = [realistic_information(rng, 300) if realistic else np.eye(6) for _ in range(n_ring)]
    info_chord = [realistic_information(rng, 200) if realistic else np.eye(6) for _ in chords]
    edges = []
    for i in range(n_ring):
        s, t = (i + 1) % n, i
        edges.append((s, t, G.inverse(truth[t]) @ truth[s], info_ring[i], False))
    for k, (a, b) in enumerate(chords):
        X = G.inverse(truth[a]) @ truth[b]
        if k in gross:
            X = X @ pose([1.0, -0.5, 0.3], 30.0, [0.6, -0.64, 0.48])
        edges.append((b, a, X, info_chord[k], True))
    start = truth.copy()
    for i in range(n):
        xi = np.concatenate([rng.normal(0, angle, 3), rng.normal(0, shift, 3)])
        if i != ref:
            start[i] = G.V(xi) @ truth[i]
    return start, edges


def _ring_case(gross):
    _, start, edges = ring(gross=gross)
    return start, edges


def _multi_edge():
    """Class 7: two edges on the ordered pair (2, 1), one on the reversed pair (1, 2), and node 5 of 6 without an edge."""
    start, edges = graph(2, n=5, chords=((0, 2),), closed=False)
    s, t, X, L, _ = edges[1]  # 2 -> 1
    assert (s, t) == (2, 1)
    edges.append((2, 1, X, 2.0 * np.eye(6), True))
    edges.append((1, 2, G.inverse(X), 0.5 * np.eye(6), False))
    lone = pose([1.0, 0.0, 0.3], 25.0, [3.0, -2.0, 1.0])
    return np.concatenate([start, lone[None]]), edges


def _negative_information():
    """Class 8: L = -I on the seven certain edges alone: every factorisation fails."""
    start, edges = graph(1, chords=())
    return start, [(s, t, X, -np.eye(6), u) for s, t, X, _, u in edges]


SIZE_SEEDS = {4: 3, 128: 2}  # seeds other than 1, where seed 1 misses a margin condition


def _sized(n):
    chords = tuple((i, i + n // 2) for i in range(0, n // 2, max(1, n // 8))) if n >= 4 else ()
    return lambda: graph(SIZE_SEEDS.get(n, 1), n=n, chords=chords)


def _sizes():
    T = tile_constant()
    out = []
    for edge in (T, 2 * T):  # N = 6 (n - 1) just below and just above the edge
        out += [(edge - 1) // 6 + 1, edge // 6 + 2]
    k = next((k for k in range(1, 200) if (k * T) % 6 == 0 and k * T // 6 + 1 <= 128), None)
    if k:
        out.append(k * T // 6 + 1)
    return sorted(set(n for n in out if n >= 2)) + [128]


# name -> (builder of (start poses, edges), options)
CASES = {
    "n2_m1": (lambda: graph(1, n=2, chords=(), closed=False), {}),
    "consistent": (lambda: _ring_case(None), {}),
    "gross_chord": (lambda: _ring_case(1), {}),
    "reference_3": (lambda: graph(1, gross=(1,), ref=3), dict(reference_node=3)),
    "reference_last": (lambda: graph(1, gross=(1,), ref=6), dict(reference_node=6)),
    # a trial in pass two as well (trials [3, 1]): the second pass's lam and gain ratio are compared too
    "second_pass_trial": (lambda: graph(3, gross=(1,), ref=6), dict(reference_node=6)),
    "far_start": (lambda: graph(4, gross=(1,), angle=0.8, shift=0.5), {}),
    "realistic": (lambda: graph(3, gross=(1,), angle=0.3, shift=0.3, realistic=True), {}),
    "multi_edge": (_multi_edge, {}),
    "negative_information": (_negative_information, {}),
    "max_iteration_1": (lambda: _ring_case(None), dict(max_iteration=1)),
    "no_pruning": (lambda: _ring_case(1), dict(edge_prune_threshold=0.0)),
    "trivial_one_node": (lambda: (graph(1)[0][:1], []), {}),
    "trivial_no_edge": (lambda: (graph(1)[0], []), {}),
}
SIZE_CASES = ["size_%d" % n for n in _sizes()]
for _n in _sizes():
    CASES["size_%d" % _n] = (_sized(_n), {})
TRIVIAL = ("trivial_one_node", "trivial_no_edge")
LINEARIZE_CASES = ["n2_m1", "consistent", "gross_chord", "realistic", "multi_edge"] + SIZE_CASES


@functools.lru_cache(maxsize=None)
def build(name):
    start, edges = CASES[name][0]()
    return np.ascontiguousarray(start, dtype=np.float64), edges, dict(G.DEFAULTS, **CASES[name][1])


def trials_of(out):
    """Per pass: the trial rows of the restatement's trace (rho None: the factorisation failed)."""
    return [[row for row in p["trace"] if row["kind"] == "trial"] for p in out["passes"]]


def reference_of(start, edges, opt):
    """The restatement's result on a graph in float64 and in longdouble."""
    return (G.global_optimization(start, edges, opt, dtype=np.float64),
            G.global_optimization(start, edges, opt, dtype=np.longdouble))


@functools.lru_cache(maxsize=None)
def reference(name):
    """reference_of a named scenario, computed once per process."""
    return reference_of(*build(name))


def decisions(out):
    flags = [[(t["accepted"], t["rho"] is not None) for t in rows] for rows in trials_of(out)]
    return dict(status=out["status"], iterations=list(out["iterations"]), flags=flags, pruned=out["pruned"].tolist())


def margin_problems(name, out64, outld, opt, edges=None):
    """Every way in which a scenario (a named one, or the graph whose `edges` are given) fails the margin conditions;
    empty when it may be used."""
    bad = []
    for p in out64["passes"]:
        for row in p["trace"]:
            if row["kind"] == "trial":
                if row["rho"] is not None and not abs(row["rho"]) >= 1e-3:
                    bad.append("gain ratio %r" % row)
            elif not row["fires"]:
                ratio = row["value"] / row["threshold"]
                if not (ratio >= 2 or ratio <= 0.5):
                    bad.append("stop test %r" % row)
    if out64["passes"] and opt["edge_prune_threshold"] > 0:
        for k, E in enumerate(build(name)[1] if edges is None else edges):
            if E[4]:
                ratio = float(out64["passes"][0]["l"][k]) / opt["edge_prune_threshold"]
                if not (ratio >= 2 or ratio <= 0.5):
                    bad.append("edge %d: l %.3g against the pruning threshold" % (k, out64["passes"][0]["l"][k]))
    if decisions(out64) != decisions(outld):
        bad.append("float64 and longdouble decide differently")
    return bad


def tolerance(q64, qld):
    """The comparison rule: 16 x the restatement's own rounding noise, never anything measured on the code under test."""
    q64, qld = np.asarray(q64, dtype=np.longdouble), np.asarray(qld, dtype=np.longdouble)
    if qld.size == 0:
        return 0.0
    return 16.0 * max(float(np.abs(q64 - qld).max()), 2.0 ** -52 * float(np.abs(qld).max()))


def ratio(got, q64, qld):
    """|got - q_longdouble| over the noise (tolerance / 16): the figure the tests print; the rule asks <= 16."""
    qld = np.asarray(qld, dtype=np.longdouble)
    if qld.size == 0:
        return 0.0
    err = float(np.abs(np.asarray(got, dtype=np.longdouble) - qld).max())
    tol = tolerance(q64, qld)
    return err / (tol / 16.0) if tol > 0 else (0.0 if err == 0 else np.inf)


def packed(name):
    """The arrays of one graph as the C ABI takes them."""
    start, edges, opt = build(name)
    m = len(edges)
    return dict(poses=start, source=np.array([E[0] for E in edges], dtype=np.int32),
                target=np.array([E[1] for E in edges], dtype=np.int32),
                transformation=np.array([E[2] for E in edges], dtype=np.float64).reshape(m, 4, 4),
                information=np.array([E[3] for E in edges], dtype=np.float64).reshape(m, 6, 6),
                uncertain=np.array([E[4] for E in edges], dtype=np.uint8), option=opt)


def write_graph_file(path, name):
    """The graph file tests/posegraph_emulation.cpp reads (repr of a float64 round-trips)."""
    start, edges, opt = build(name)
    with open(path, "w") as f:
        f.write("%d %d\n" % (len(start), len(edges)))
        f.write(" ".join(repr(opt[k]) for k in G.DEFAULTS) + "\n")
        for T in start:
            f.write(" ".join(repr(float(v)) for v in T.ravel()) + "\n")
        for s, t, X, L, unc in edges:
            f.write("%d %d %d " % (s, t, int(unc)) + " ".join(repr(float(v)) for v in np.asarray(X).ravel()) + " " +
                    " ".join(repr(float(v)) for v in np.asarray(L, dtype=np.float64).ravel()) + "\n")


def check_against_reference(name, got, report=print, graph=None, refs=None):
    """`got`: dict(status, iterations, trials, flags (per pass, (accepted, factorised) per trial), pruned, poses,
    confidence, F0, F, mu (per pass), lam (per pass, per trial)) of an implementation.  Decisions must EQUAL the
    restatement's; numbers are compared with the longdouble restatement under the rule.  Returns the ratios.  A graph
    that is no named scenario is given as graph = (start, edges, opt) with refs = reference_of(*graph)."""
    o64, old = reference(name) if refs is None else refs
    start, edges, opt = build(name) if graph is None else graph
    want = decisions(o64)
    tr64, trld = trials_of(o64), trials_of(old)
    assert got["status"] == want["status"], (name, got["status"], want["status"])
    assert list(got["iterations"]) == want["iterations"], (name, got["iterations"], want["iterations"])
    n_pass = len(o64["passes"])
    assert list(got["trials"]) == [len(tr64[p]) if p < n_pass else 0 for p in range(2)], (name, got["trials"])
    assert [list(map(tuple, f)) for f in got["flags"][:n_pass]] == want["flags"], (name, got["flags"], want["flags"])
    assert [bool(x) for x in got["pruned"]] == want["pruned"], name
    ref = 0 if opt["reference_node"] < 0 else opt["reference_node"]
    if len(start):
        assert np.array_equal(np.asarray(got["poses"])[ref], start[ref]), name
    q = dict(poses=(o64["poses"], old["poses"]), confidence=(o64["confidence"], old["confidence"]),
             F0=(o64["F0"], old["F0"]), F=(o64["F"], old["F"]),
             mu=([p["mu"] for p in o64["passes"]], [p["mu"] for p in old["passes"]]),
             lam=([t["lam"] for rows in tr64 for t in rows], [t["lam"] for rows in trld for t in rows]))
    mine = dict(got, mu=list(got["mu"])[:n_pass], lam=[v for rows in got["lam"][:n_pass] for v in rows])
    ratios = {}
    for key, (a64, ald) in q.items():
        ratios[key] = ratio(np.asarray(mine[key], dtype=np.float64), np.asarray(a64, dtype=np.longdouble),
                            np.asarray(ald, dtype=np.longdouble))
    report("posegraph %-22s ratio to the restatement's noise: " % name +
           " ".join("%s %.3g" % (k, v) for k, v in ratios.items()))
    for key, v in ratios.items():
        assert v <= 16.0, (name, key, v)
    return ratios


WIDE_BATCH = 320
WIDE_LARGE = 256  # where the 128-node graph stands in the wide batch


def wide_batch():
    """The names of 320 scenarios for one call: the sized cases of 3, 4, 6, 7 and 9 nodes in turn (the 3-node ring has
    no uncertain edge, so Levenberg-Marquardt runs without a line process there and with one elsewhere) and the 128-node
    graph, the tile-edge case, at WIDE_LARGE.  What the wide test rests on is asserted from the sizes alone."""
    small = [n for n in SIZE_CASES if n != "size_128"]
    names = [small[i % len(small)] for i in range(WIDE_BATCH)]
    names[WIDE_LARGE] = "size_128"
    assert len(names) > 256 and len(small) == 5  # one workgroup per graph: blockIdx.x past 255
    nodes = [len(build(n)[0]) for n in names]
    edges = [len(build(n)[1]) for n in names]
    assert len({nodes[255], nodes[256], nodes[257]}) == 3 and nodes[256] == 128
    assert len(set(nodes[:5])) == 5 and len(set(edges[:5])) == 5  # no stride by a constant graph size can be right
    uncertain = [any(E[4] for E in build(n)[1]) for n in small]
    assert any(uncertain) and not all(uncertain)
    return names
