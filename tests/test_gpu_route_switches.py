"""Every route switch and tuning knob of teaser_hip_set_option (tests/route_matrix.py: ROUTES, COMBOS) against the
default route in the same process, bit for bit, and against the oracle, on the workload of its stage.  Each test also
asserts that the route it claims to test was taken.  Run on a real MI355X with `pytest -m gpu`."""
import hashlib
import importlib
import json
import os
from contextlib import contextmanager

import numpy as np
import pytest

import route_matrix as rm
from oracle import oracle
from util import ROOT, HipBuffers, is_clique

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")
ROWS = rm.setting_rows()
TIME_LIMIT = 5  # TEASER_HIP_STATUS of a search ended by max_clique_time_limit


@pytest.fixture(autouse=True)
def _restore_options():
    """Options are process-wide: every test starts from, and leaves, the values it found."""
    saved = {name: tp.get_option(name) for name in ROWS}
    yield
    for name, v in saved.items():
        if tp.get_option(name) != v:
            tp.set_option(name, v)


@contextmanager
def options(opts):
    before = {k: tp.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            tp.set_option(k, v)
        yield
    finally:
        for k, v in before.items():
            tp.set_option(k, v)


def cases(*names):
    """(option, value) of ROUTES for these options, without the default value (that is the reference route)."""
    return [pytest.param(n, v, id="%s=%d" % (n, v)) for n in names for v in rm.ROUTES[n] if v != ROWS[n][1]]


def make_solver(**kw):
    return tp.RobustRegistrationSolver(tp.RobustRegistrationSolver.Params(**kw))


def bench_params(**kw):
    p = dict(noise_bound=0.01, cbar2=1.0, estimate_scaling=False, rotation_gnc_factor=1.4,
             rotation_max_iterations=100, rotation_cost_threshold=0.005)
    p.update(kw)
    return p


def oracle_params(p):
    return dict(p, estimate_scaling=int(p.get("estimate_scaling", True)))


def result(s, b=0):
    """Everything a problem's solve returns, in a form that compares bit for bit."""
    r = s.raw_solution(b)
    return dict(valid=int(r.valid), status=int(r.status), scale=np.float64(r.scale).tobytes(),
                R=np.array(r.rotation[:], dtype=np.float64).tobytes(), t=np.array(r.translation[:], dtype=np.float64).tobytes(),
                size=int(r.clique_size), heuristic=int(r.heuristic_size), uncoloured=int(r.colour_uncoloured),
                exact=int(r.clique_exact_run), edges=int(r.num_edges), clique=s.getInlierMaxClique(b),
                rot=s.getRotationInliers(b) if r.valid else None, trans=s.getTranslationInliers(b) if r.valid else None)


def assert_same(got, want, what, content=True):
    """content=False: a maximum clique that is not unique may differ (the exact search records the first one it
    finds); the size, the edges and the verdict may not."""
    keys = list(want) if content else ["valid", "status", "size", "edges"]
    diff = [k for k in keys if got[k] != want[k]]
    assert not diff, (what, diff, [(got[k], want[k]) for k in diff if k not in ("R", "t", "scale")])


def bitmap_rows_popcount(bm):
    return np.unpackbits(np.ascontiguousarray(bm).view(np.uint8), axis=1).sum(1)


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


@pytest.fixture(autouse=True, scope="module")
def _release_cache():
    yield
    _CACHE.clear()


# ---------------------------------------------------------------------------------------------
# K1 fix-up: fixup_wgs
# ---------------------------------------------------------------------------------------------
def k1_only_params(nb):
    return bench_params(noise_bound=nb, inlier_selection_mode=tp.InlierSelectionMode.PMC_HEU, max_clique_time_limit=5.0)


def k1_cases():
    """(name, noise bound, problems solved as one batch): test_k1_filter_adversarial_band's problems (many flagged
    groups), test_k1_filter_fallbacks' worklist overflow beside a normal problem (the host reruns the batch on the
    FP64 K1) and a beta the filter cannot resolve (the FP64 body inside K1, degrees counted by the fix-up)."""
    out = []
    rng = np.random.default_rng(17)
    for scale, nb in ((1.0, 0.01), (250.0, 0.05), (0.02, 1e-4)):
        beta = 2 * nb
        n = 2048
        src = rng.uniform(-1, 1, size=(3, n)) * scale
        R0 = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        dst = R0 @ src
        off = rng.choice([0, 1, -1], size=n) * beta * (1 + rng.choice([0, 1e-15, 1e-12, 1e-9, 1e-7, 1e-5, 1e-3], size=n))
        d = dst / np.linalg.norm(dst, axis=0)
        dst = dst + d * off * rng.uniform(0.3, 1.0, size=n)
        out.append(("band_%g" % scale, nb, [(src, dst)]))
    rng = np.random.default_rng(14)
    base = rng.uniform(size=(3, 6))
    idx = rng.integers(0, 6, size=3000)
    src = base[:, idx] + rng.uniform(-1e-4, 1e-4, size=(3, 3000))
    dst = src + rng.uniform(-2e-3, 2e-3, size=src.shape)
    prn = tp.synth_problem(20250523 + 18, 2000, 0.9, 0.01)
    out.append(("overflow", 0.01, [(src, dst), (prn["src"], prn["dst"])]))
    pr = tp.synth_problem(20250523 + 15, 700, 0.5, 1e-7)
    out.append(("fp64_body", 1e-7, [(pr["src"], pr["dst"])]))
    return out


def run_k1_cases():
    got = {}
    for name, nb, probs in cached("k1_cases", k1_cases):
        s = make_solver(**k1_only_params(nb))
        s.set_profiling(1)
        s.solve_batch([p[0] for p in probs], [p[1] for p in probs])
        prof = s.get_profile()
        got[name] = [(result(s, b), s.getInlierGraphBitmap(b), s.getDegrees(b)) for b in range(len(probs))]
        got[name].append((prof["tim_graph_launches"], prof["tim_aux_ms"]))
        s.close()
    return got


def k1_oracle():
    out = {}
    for name, nb, probs in cached("k1_cases", k1_cases):
        out[name] = []
        for src, dst in probs:
            _, ref = oracle.inlier_bitmap(src, dst, nb, 1.0, False)
            out[name].append((ref, oracle.bitmap_to_dense(ref, src.shape[1]).sum(1)))
    return out


def headline(opts):
    fx = cached("c2", lambda: json.load(open(os.path.join(ROOT, "tests", "golden", "config2_batch_golden.json"))))
    probs = cached("c2_probs", lambda: [tp.synth_problem(fx["seed0"] + b, fx["n"], fx["outlier_ratio"], fx["noise_bound"])
                                        for b in range(fx["batch"])])
    with options(opts):
        s = make_solver(**bench_params())
        s.set_profiling(1)
        s.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
        prof = s.get_profile()
        res = [result(s, b) for b in range(len(probs))]
        bms = {b: np.ascontiguousarray(s.getInlierGraphBitmap(b)) for b in (0, 17, 30, 63)}
        degs = {b: s.getDegrees(b) for b in bms}
        s.close()
    return fx, res, bms, degs, prof


@pytest.mark.parametrize("name,value", cases("fixup_wgs"))
def test_fixup_wgs(name, value):
    want = cached("k1_default", run_k1_cases)
    ref = cached("k1_oracle", k1_oracle)
    with options({name: value}):
        got = run_k1_cases()
    for case in got:
        launches, aux_ms = got[case][-1]
        assert launches == want[case][-1][0] and aux_ms > 0.0, (case, launches, aux_ms)  # the fix-up ran (K1 phase 2)
        for b, (r, bm, deg) in enumerate(got[case][:-1]):
            assert (bm == ref[case][b][0]).all(), (case, b)
            assert (deg == ref[case][b][1]).all(), (case, b)
            assert_same(r, want[case][b][0], (case, b))
    assert got["overflow"][-1][0] == 2  # the overflow: the matrix-core K1, then the rerun on the FP64 K1
    fx, res, bms, degs, prof = headline({name: value})
    _, want_res, _, _, _ = cached("headline_default", lambda: headline({}))
    assert prof["tim_graph_launches"] == 1 and prof["tim_aux_ms"] > 0.0
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.int32)).tobytes()).hexdigest()
    for b, f in enumerate(fx["problems"]):
        assert_same(res[b], want_res[b], b)
        assert res[b]["edges"] == f["num_edges"] and res[b]["size"] == f["clique_size"], b
        if f["clique_unique"]:
            assert sha(res[b]["clique"]) == f["max_clique_sha256"], b
            assert sha(res[b]["rot"]) == f["rotation_inliers_sha256"], b
            assert sha(res[b]["trans"]) == f["translation_inliers_sha256"], b
    for b, bm in bms.items():
        assert hashlib.sha256(bm.tobytes()).hexdigest() == fx["problems"][b]["bitmap_sha256"], b
        assert (degs[b] == bitmap_rows_popcount(bm)).all(), b


# ---------------------------------------------------------------------------------------------
# heuristic and degree closure: heu_blocks, greedy_threads, deg_closure_wgs
# ---------------------------------------------------------------------------------------------
def heuristic_problems():
    """64 problems: the closure decides most of the 0.8 / 0.9 ones; at 95 % outliers (and noise bound 0.05 for every
    fourth) it declines and the greedy starts, the selection and the peel decide."""
    out = []
    for i in range(64):
        rho = (0.8, 0.95, 0.9, 0.95)[i % 4]
        out.append(tp.synth_problem(33000 + i, 300 + (i * 137) % 2200, rho, 0.01))
    return out


def run_heuristic(opts):
    probs = cached("heu_probs", heuristic_problems)
    out = {}
    with options(opts):
        s = make_solver(**bench_params())
        for B in (1, 16, 17, 64):
            s.solve_batch([p["src"] for p in probs[:B]], [p["dst"] for p in probs[:B]])
            out[B] = [result(s, b) for b in range(B)]
        s.close()
    return out


def heuristic_oracle():
    probs = cached("heu_probs", heuristic_problems)
    return [oracle.solve(p["src"], p["dst"], **oracle_params(bench_params())) for p in probs[:12]]


def two_clique_graph():
    """A sparse random graph of 2000 vertices with two disjoint planted 20-cliques: one on vertices = 0 mod 16, the
    other on vertices = 5 mod 16, so that start 0 (the highest-degree vertex of residue class 0) grows the first and
    start 5 the second.  The peel at 20 then empties the graph: the first start that finishes closes the problem.
    "Largest clique, ties to the lowest start" picks the first clique whatever the launch geometry."""
    rng = np.random.default_rng(91)
    n = 2000
    A = np.triu(rng.uniform(size=(n, n)) < 0.004, 1)
    c0 = np.sort(rng.choice(np.arange(0, n, 16), size=20, replace=False))
    c5 = np.sort(rng.choice(np.arange(5, n, 16), size=20, replace=False))
    for c in (c0, c5):
        A[np.ix_(c, c)] |= np.triu(np.ones((20, 20), dtype=bool), 1)
    A = A | A.T
    return A, oracle.bitmap_from_edges(n, np.argwhere(np.triu(A, 1))), c0.tolist(), c5.tolist()


def run_ties(opts):
    """The two-clique graph through maxClique and the synthetic tie (test_degree_closure_decides_a_tie_between_maximum
    _cliques' problem: two maximum cliques) alone and in a batch of 17, with the degree closure off and on."""
    A, bm, c0, c5 = cached("two_cliques", two_clique_graph)
    tie = cached("tie", lambda: tp.synth_problem(20250523 + 30, 10000, 0.95, 0.01))
    probs = cached("heu_probs", heuristic_problems)[:16]
    out = {}
    for closure in (0, 1):
        with options(dict(opts, deg_closure=closure)):
            s = make_solver(**bench_params())
            c, er = s.maxClique(bm, A.shape[0])
            out[("graph", closure)] = (c, er, s.last_status)
            s.solve(tie["src"], tie["dst"])
            out[("tie", closure)] = result(s)
            s.solve_batch([tie["src"]] + [p["src"] for p in probs], [tie["dst"]] + [p["dst"] for p in probs])
            out[("tie17", closure)] = result(s, 0)
            s.close()
    return out


def check_ties(got, want):
    A, _, c0, c5 = cached("two_cliques", two_clique_graph)
    for closure in (0, 1):
        c, er, status = got[("graph", closure)]
        assert len(c) == 20 and is_clique(A, c) and c in (c0, c5), closure
        assert (c, er, status) == want[("graph", closure)], closure
        for k in ("tie", "tie17"):
            assert_same(got[(k, closure)], want[(k, closure)], (k, closure), content=got[(k, closure)]["exact"] == 0)
    assert got[("graph", 0)][0] == c0  # the lowest start's clique
    r = got[("tie", 0)]
    assert r["uncoloured"] not in (-2, -3)  # closure off: the greedy starts' clique was returned
    assert got[("tie", 1)]["uncoloured"] == -3  # closure on: decided among the two by the closure
    tie_o = cached("tie_oracle", lambda: oracle.solve(cached("tie", None)["src"], cached("tie", None)["dst"],
                                                      **oracle_params(bench_params())))
    assert not tie_o["clique_unique"] and r["size"] == len(tie_o["max_clique"]) and r["edges"] == tie_o["num_edges"]


def check_heuristic(got, want, ref):
    open_heu = 0
    for B in got:
        for b in range(B):
            assert_same(got[B][b], want[B][b], (B, b))
            open_heu += int(got[B][b]["uncoloured"] not in (-2, -3))
    decided = sum(int(r["uncoloured"] == -2) for r in got[64])
    assert open_heu >= 4 and decided >= 4, (open_heu, decided)  # both routes of the batch were exercised
    for b, o in enumerate(ref):
        r = got[64][b]
        assert r["size"] == len(o["max_clique"]) and r["edges"] == o["num_edges"], b
        if o["clique_unique"]:
            assert r["clique"] == o["max_clique"].tolist() and r["rot"] == o["rotation_inliers"].tolist(), b
            assert r["trans"] == o["translation_inliers"].tolist(), b


@pytest.mark.parametrize("name,value", cases("heu_blocks", "greedy_threads", "deg_closure_wgs"))
def test_heuristic_geometry(name, value):
    """Batches of 1, 16, 17 and 64 problems (both sides of the 16- and 64-problem thresholds of
    heuristic_blocks_per_problem and launch_heuristic) and the maximum-clique ties."""
    want = cached("heu_default", lambda: run_heuristic({}))
    ref = cached("heu_oracle", heuristic_oracle)
    check_heuristic(run_heuristic({name: value}), want, ref)
    check_ties(run_ties({name: value}), cached("ties_default", lambda: run_ties({})))


def test_heuristic_wide_combo_on_64_problems():
    """COMBOS["wide_heuristic_64"]: 16 workgroups of 512 threads per problem on a 64-problem batch."""
    combo = rm.COMBOS["wide_heuristic_64"]
    want = cached("heu_default", lambda: run_heuristic({}))
    check_heuristic(run_heuristic(combo), want, cached("heu_oracle", heuristic_oracle))
    check_ties(run_ties(combo), cached("ties_default", lambda: run_ties({})))


def test_two_clique_tie_goes_to_the_lowest_start():
    """The default route itself: the two-clique graph's answer is the clique of start 0, alone and whatever the
    number of workgroups (heu_blocks 1 and 16 bracket the geometry)."""
    A, bm, c0, c5 = cached("two_cliques", two_clique_graph)
    o = oracle.max_clique(bm, A.shape[0])
    assert len(o["clique"]) == 20 and not o["unique"]
    for hb in (0, 1, 16):
        with options(dict(heu_blocks=hb, deg_closure=0)):
            s = make_solver(**bench_params())
            c, er = s.maxClique(bm, A.shape[0])
            s.close()
        assert c == c0 and not er, hb


# ---------------------------------------------------------------------------------------------
# exact search: k4_*, greedy_small
# ---------------------------------------------------------------------------------------------
K4_OPTIONS = ("k4_lds_stack", "k4_donate", "k4_donate_after", "k4_hungry", "k4_expand", "k4_waves")


def config5():
    C5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    A, B, vox = C5["cloud_bin_0"], C5["cloud_bin_4"], float(C5["voxel_size"])
    est = tp.FPFHEstimation()
    fa = est.computeFPFHFeatures(A, 2 * vox, 5 * vox)
    fb = est.computeFPFHFeatures(B, 2 * vox, 5 * vox)
    corr = tp.Matcher().calculateCorrespondences(A, B, fa, fb, False, True, False, 0)
    c = np.array(corr)
    g5 = json.load(open(os.path.join(ROOT, "tests", "golden", "config5_result_golden.json")))
    assert g5["correspondences_sha256"] == hashlib.sha256(np.ascontiguousarray(c, dtype=np.int32).tobytes()).hexdigest()
    src = np.ascontiguousarray(A[c[:, 0]].astype(np.float64).T)
    dst = np.ascontiguousarray(B[c[:, 1]].astype(np.float64).T)
    p = dict(noise_bound=vox, cbar2=1.0, estimate_scaling=False, rotation_gnc_factor=1.4,
             rotation_max_iterations=10000, rotation_cost_threshold=1e-16, max_clique_time_limit=30.0)
    _, bm = oracle.inlier_bitmap(src, dst, vox, 1.0, False)
    dense = np.unpackbits(bm.view(np.uint8), axis=1, bitorder="little")[:, :src.shape[1]].astype(bool)
    # 16 distinct members: a fixed random 3 % of the correspondences dropped from each
    rng = np.random.default_rng(555)
    members = []
    for k in range(16):
        keep = np.sort(rng.choice(src.shape[1], size=src.shape[1] - int(0.03 * src.shape[1]), replace=False))
        members.append((np.ascontiguousarray(src[:, keep]), np.ascontiguousarray(dst[:, keep])))
    return g5, src, dst, p, dense, members


def config5_member_oracle():
    _, _, _, p, _, members = cached("c5", config5)
    q = dict(p, estimate_scaling=0)
    q.pop("max_clique_time_limit")
    return [oracle.solve(m[0], m[1], **q) for m in members]


def clique_graphs():
    """maxClique workloads: test_planted_clique_needs_exact's graph, six of test_colouring_bound_and_restricted_roots'
    graphs, and the 1020- and 1080-vertex graphs of test_mid_size_graph_cliques_vs_oracle (both sides of the
    1024-vertex LDS adjacency)."""
    out = []
    rng = np.random.default_rng(15)
    n, k = 400, 30
    A = np.triu(rng.uniform(size=(n, n)) < 0.35, 1)
    m = np.sort(rng.choice(n, size=k, replace=False))
    A[np.ix_(m, m)] |= np.triu(np.ones((k, k), dtype=bool), 1)
    out.append(("planted", n, A))
    rng = np.random.default_rng(77)
    for trial in range(6):
        n = int(rng.integers(120, 700))
        p = float(rng.uniform(0.1, 0.45))
        A = np.triu(rng.uniform(size=(n, n)) < p, 1)
        for _ in range(int(rng.integers(1, 5))):
            k = int(rng.integers(8, 40))
            m = rng.choice(n, size=k, replace=False)
            A[np.ix_(m, m)] |= True
            A = np.triu(A, 1)
        out.append(("colouring_%d" % trial, n, A))
    rng = np.random.default_rng(16)
    for n, p in ((600, 0.12), (760, 0.10), (900, 0.08), (1020, 0.08), (1080, 0.07)):
        A = np.triu(rng.uniform(size=(n, n)) < p, 1)
        m = np.sort(rng.choice(n, size=9, replace=False))
        A[np.ix_(m, m)] |= np.triu(np.ones((9, 9), dtype=bool), 1)
        if n >= 1020:
            out.append(("mid_%d" % n, n, A))
    res = []
    for name, n, A in out:
        bm = oracle.bitmap_from_edges(n, np.argwhere(A))
        res.append((name, n, A | A.T, bm, oracle.max_clique(bm, n)))
    return res


def run_exact(opts, capfd):
    """config 5 with greedy_small = 0 (the heuristic stops at 91: the exact search must find 92) alone, x 64 through
    solve_batch and submit_batch, the 16 distinct members; then the supplied graphs.  Returns the results and the
    exact-search diagnostics line of the single solve (k4_debug on for that solve only)."""
    g5, src, dst, p, dense, members = cached("c5", config5)
    out = {}
    opts = dict(opts)
    opts.setdefault("greedy_small", 0)
    with options(opts):
        s = make_solver(**p)
        capfd.readouterr()
        with options({"k4_debug": 1}):
            s.solve(src, dst)
        err = capfd.readouterr().err
        out["single"] = result(s)
        s.solve_batch([src] * 64, [dst] * 64)
        out["batch64"] = [result(s, b) for b in range(64)]
        mem = HipBuffers()
        packed_src = np.ascontiguousarray(np.concatenate([src.T] * 64, axis=0))
        packed_dst = np.ascontiguousarray(np.concatenate([dst.T] * 64, axis=0))
        nn = np.full(64, src.shape[1], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(nn)[:-1]]).astype(np.int64)
        t = s.submit_batch(mem.device(packed_src), mem.device(packed_dst), off, nn)
        sols = s.wait(t)
        out["submit64"] = [dict(valid=int(o.valid), status=int(o.status), size=int(o.clique_size),
                                edges=int(o.num_edges), exact=int(o.clique_exact_run), heuristic=int(o.heuristic_size),
                                clique=s.getInlierMaxClique(b)) for b, o in enumerate(sols[:64])]
        s.solve_batch([m[0] for m in members], [m[1] for m in members])
        out["members"] = [result(s, b) for b in range(16)]
        graphs = []
        for name, n, A, bm, o in cached("graphs", clique_graphs):
            c, er = s.maxClique(bm, n)
            graphs.append((name, c, er, s.last_status))
        out["graphs"] = graphs
        s.close()
        mem.free()
    return out, [ln for ln in err.splitlines() if "exact search:" in ln]


def check_exact(got, dbg, name=None, value=None):
    g5, src, dst, p, dense, members = cached("c5", config5)
    assert len(dbg) >= 1, dbg
    line = dbg[0]
    assert ("donation queue OFF" in line) == (name == "k4_donate" and value == 0 or name == "hbm_records_no_donation"), line
    if name == "k4_lds_stack":
        assert ("LDS stack %d B" % (value & ~15 if value <= 16384 else 0)) in line, line
    if name == "k4_expand":
        assert ("%d expansion passes" % min(value, 7)) in line, line
    if name == "k4_waves":  # (the default is 4096 persistent waves, or one per root when there are more roots)
        default_line = cached("exact_default", None)[1][0]
        assert line.split()[-2] != default_line.split()[-2], (line, default_line)
    for r in [got["single"]] + got["batch64"] + got["submit64"]:
        assert r["valid"] and r["status"] != TIME_LIMIT and r["exact"] == 1, r["status"]
        assert r["heuristic"] == 91 and r["size"] == g5["clique_size"] == 92 and r["edges"] == g5["num_edges"]
        c = np.asarray(r["clique"])
        assert dense[np.ix_(c, c)].sum() == len(c) * (len(c) - 1)  # a clique of the oracle's graph
    ref = cached("c5_members_oracle", config5_member_oracle)
    for b, (r, o) in enumerate(zip(got["members"], ref)):
        assert r["status"] != TIME_LIMIT and r["size"] == len(o["max_clique"]) and r["edges"] == o["num_edges"], b
        if o["clique_unique"]:
            assert r["clique"] == o["max_clique"].tolist(), b
    assert sum(r["exact"] for r in got["members"]) >= 1  # the exact search ran across several distinct problems
    n_exact = 0
    for (name_g, c, er, status), (_, n, A, bm, o) in zip(got["graphs"], cached("graphs", clique_graphs)):
        assert status != TIME_LIMIT and len(c) == len(o["clique"]) and is_clique(A, c) and c == sorted(c), name_g
        if o["unique"]:
            assert c == o["clique"].tolist(), name_g
        n_exact += int(er)
    assert n_exact >= 1


def compare_exact(got, want):
    """Against the default route: everything but the content of a maximum clique that is not unique."""
    for k in ("single",):
        assert_same(got[k], want[k], k, content=False)
    for k in ("batch64", "submit64"):
        for b in range(64):
            assert_same(got[k][b], want[k][b], (k, b), content=False)
    ref = cached("c5_members_oracle", config5_member_oracle)
    for b, o in enumerate(ref):
        assert_same(got["members"][b], want["members"][b], ("member", b), content=bool(o["clique_unique"]))
    for g, w, (_, _, _, _, o) in zip(got["graphs"], want["graphs"], cached("graphs", clique_graphs)):
        assert len(g[1]) == len(w[1]) and (g[1] == w[1] or not o["unique"]), g[0]


@pytest.mark.parametrize("name,value", cases(*K4_OPTIONS))
def test_exact_search_routes(name, value, capfd):
    want = cached("exact_default", lambda: run_exact({}, capfd))
    got, dbg = run_exact({name: value}, capfd)
    capfd.readouterr()
    check_exact(got, dbg, name, value)
    compare_exact(got, want[0])


@pytest.mark.parametrize("combo", ["max_donation_traffic", "hbm_records_no_donation"])
def test_exact_search_combos(combo, capfd):
    want = cached("exact_default", lambda: run_exact({}, capfd))
    got, dbg = run_exact(rm.COMBOS[combo], capfd)
    check_exact(got, dbg, combo)
    compare_exact(got, want[0])


def test_exact_search_default_route_and_greedy_small(capfd):
    """The reference route of the tests above (greedy_small = 0) checked on its own, and greedy_small = 1: the
    all-starts greedy finds 92 on config 5 and the exact search is not needed there."""
    want, dbg = cached("exact_default", lambda: run_exact({}, capfd))
    check_exact(want, dbg)
    g5, src, dst, p, dense, _ = cached("c5", config5)
    with options({"greedy_small": 1}):
        s = make_solver(**p)
        s.solve(src, dst)
        r = result(s)
        s.close()
    assert r["heuristic"] == r["size"] == 92 and r["edges"] == g5["num_edges"]
    c = np.asarray(r["clique"])
    assert dense[np.ix_(c, c)].sum() == len(c) * (len(c) - 1)


# ---------------------------------------------------------------------------------------------
# scale stage: scale_batch, scale_mid_batch
# ---------------------------------------------------------------------------------------------
def scale_sets():
    """The problem sets of test_estimate_scaling_batch_small_problems and _mid_size_problems."""
    nb = 0.01
    small = []
    for i, n in enumerate([60, 300, 724, 2, 511, 900, 128, 725, 1]):
        q = tp.synth_problem(500 + i, n, 0.5, nb)
        small.append((q["src"], q["dst"] * (1.0 + 0.25 * i)))
    mid = []
    for i, n in enumerate([800, 1500, 2000, 900, 1000, 3000, 725]):
        q = tp.synth_problem(700 + i, n, 0.6, nb)
        mid.append((q["src"], q["dst"] * (0.5 + 0.3 * i)))
    return [("small", small, bench_params(estimate_scaling=True, noise_bound=nb * 3.25), (1, 4)),
            ("mid", mid, bench_params(estimate_scaling=True, noise_bound=nb * 2.5), (0,))]


def run_scale(opts, capfd):
    out = {}
    lines = []  # the first scale-stage diagnostics line of each set
    with options(dict(opts, k4_debug=0)):
        for name, probs, p, _ in cached("scale_sets", scale_sets):
            s = make_solver(**p)
            capfd.readouterr()
            with options({"k4_debug": 1}):
                s.solve_batch([q[0] for q in probs], [q[1] for q in probs])
            lines += [ln for ln in capfd.readouterr().err.splitlines() if "scale stage:" in ln][:1]
            out[name] = [result(s, b) for b in range(len(probs))]
            s.solve_batch([q[0] for q in probs], [q[1] for q in probs])  # and without diagnostics
            out[name + "_quiet"] = [result(s, b) for b in range(len(probs))]
            s.close()
    return out, lines


@pytest.mark.parametrize("name,value", cases("scale_batch", "scale_mid_batch"))
def test_scale_stage_routes(name, value, capfd):
    want, want_lines = cached("scale_default", lambda: run_scale({}, capfd))
    got, lines = run_scale({name: value}, capfd)
    assert len(lines) == 2 and len(want_lines) == 2, (lines, want_lines)
    # the default batches every problem above 1 point but one; the switched-off route runs more of them alone
    alone = lambda ln: int(ln.split(" batched, ")[1].split()[0])
    assert alone(lines[0 if name == "scale_batch" else 1]) > alone(want_lines[0 if name == "scale_batch" else 1]), (lines, want_lines)
    for set_name, probs, p, check in cached("scale_sets", scale_sets):
        for b in range(len(probs)):
            assert_same(got[set_name][b], want[set_name][b], (set_name, b))
            assert_same(got[set_name + "_quiet"][b], want[set_name][b], (set_name, b))
        for b in check:
            ref = cached(("scale_oracle", set_name, b), lambda: oracle.solve(probs[b][0], probs[b][1], **oracle_params(p)))
            r = got[set_name][b]
            assert abs(np.frombuffer(r["scale"])[0] - ref["scale"]) <= 1e-9 * max(1.0, abs(ref["scale"])), (set_name, b)
            assert r["clique"] == ref["max_clique"].tolist() or not ref["clique_unique"], (set_name, b)


# ---------------------------------------------------------------------------------------------
# asynchronous schedule: depth, stagger, k1_stream, tail_cus, tail_cu_block, copy_stream, h2d_kernel
# ---------------------------------------------------------------------------------------------
def async_digest(opts):
    import async_digest as ad
    with options(opts):
        return ad.run(depth=None)


def lane_evidence(opts, capfd):
    """The diagnostics of a new handle's lanes and of its host-input copies (k4_debug on, one small batch)."""
    pr = tp.synth_problem(4242, 500, 0.8, 0.01)
    mem = HipBuffers()
    src = np.ascontiguousarray(pr["src"].T)
    dst = np.ascontiguousarray(pr["dst"].T)
    with options(dict(opts, k4_debug=1)):
        s = make_solver(**bench_params())
        capfd.readouterr()
        t = s.submit_batch(mem.pinned(src), mem.pinned(dst), np.zeros(1, dtype=np.int64),
                           np.array([500], dtype=np.int32), host=True)
        s.wait(t)
        s.close()
    mem.free()
    return [ln for ln in capfd.readouterr().err.splitlines() if "lane:" in ln or "copy stream" in ln or "host inputs" in ln]


def headline_host_inputs(opts):
    """The host-input half of test_async_headline_batch_64x10k_vs_oracle_fixture."""
    fx = cached("c2", lambda: json.load(open(os.path.join(ROOT, "tests", "golden", "config2_batch_golden.json"))))
    probs = cached("c2_probs", lambda: [tp.synth_problem(fx["seed0"] + b, fx["n"], fx["outlier_ratio"], fx["noise_bound"])
                                        for b in range(fx["batch"])])
    other = cached("c2_other", lambda: [tp.synth_problem(fx["seed0"] + 500 + b, fx["n"], fx["outlier_ratio"], fx["noise_bound"])
                                        for b in range(fx["batch"])])

    def packed(ps):
        src = np.ascontiguousarray(np.concatenate([p["src"].T for p in ps], axis=0))
        dst = np.ascontiguousarray(np.concatenate([p["dst"].T for p in ps], axis=0))
        n = np.array([p["src"].shape[1] for p in ps], dtype=np.int32)
        return src, dst, np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64), n

    mem = HipBuffers()
    got = []
    with options(opts):
        s = make_solver(**bench_params())
        s.set_pipeline_depth(2)
        sa, da, off, nn = packed(probs)
        sb, db, _, _ = packed(other)
        A = (mem.pinned(sa), mem.pinned(da))
        Bb = (mem.pinned(sb), mem.pinned(db))
        t0 = s.submit_batch(A[0], A[1], off, nn, host=True)
        t1 = s.submit_batch(Bb[0], Bb[1], off, nn, host=True)
        s.wait(t0)
        got.append([result(s, b) for b in range(len(probs))] + [hashlib.sha256(np.ascontiguousarray(s.getInlierGraphBitmap(b)).tobytes()).hexdigest() for b in (0, 30, 63)])
        t2 = s.submit_batch(A[0], A[1], off, nn, host=True)
        s.wait(t1)
        s.wait(t2)
        got.append([result(s, b) for b in range(len(probs))] + [hashlib.sha256(np.ascontiguousarray(s.getInlierGraphBitmap(17)).tobytes()).hexdigest()])
        s.close()
    mem.free()
    return fx, got


def check_headline_host(fx, got):
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.int32)).tobytes()).hexdigest()
    for res, bms in ((got[0][:-3], dict(zip((0, 30, 63), got[0][-3:]))), (got[1][:-1], {17: got[1][-1]})):
        for b, f in enumerate(fx["problems"]):
            r = res[b]
            assert bool(r["valid"]) == f["valid"] and r["edges"] == f["num_edges"] and r["size"] == f["clique_size"], b
            if f["clique_unique"]:
                assert sha(r["clique"]) == f["max_clique_sha256"] and sha(r["rot"]) == f["rotation_inliers_sha256"], b
                assert sha(r["trans"]) == f["translation_inliers_sha256"], b
        for b, h in bms.items():
            assert h == fx["problems"][b]["bitmap_sha256"], b


def expected_lane_line(name, value):
    return {"depth": "depth %d," % value, "stagger": ("stagger 0" if value == 0 else "(point %d)" % value),
            "k1_stream": {1: "K1 stream shared,", 2: "K1 stream shared (kernel only)"}.get(value),
            "tail_cus": "tail CUs %d (spread)" % value, "tail_cu_block": "(block)"}.get(name)


@pytest.mark.parametrize("name,value", cases(*[n for n in rm.ROUTES if n in
                                               ("depth", "stagger", "k1_stream", "tail_cus", "tail_cu_block",
                                                "copy_stream", "h2d_kernel")]))
def test_async_schedule_routes(name, value, capfd):
    opts = {name: value}
    if name == "tail_cu_block":
        opts["tail_cus"] = 8  # (the block partition needs a partition)
    evidence = lane_evidence(opts, capfd)
    if name in ("copy_stream",):
        assert any(("copy stream: " + ("own" if value == 1 else "own, high priority")) == ln.split("] ")[1]
                   for ln in evidence), evidence
    elif name == "h2d_kernel":
        assert any("host inputs: kernel" in ln for ln in evidence), evidence
    else:
        want_line = expected_lane_line(name, value)
        assert any(want_line in ln for ln in evidence if "lane:" in ln), (want_line, evidence)
    want = cached("digest_default", lambda: async_digest({}))
    got = async_digest(opts)
    assert got["coloured"] >= 12 and got["exact"] == want["exact"], (got, want)
    assert got["digest"] == want["digest"], (got, want)
    if name in ("copy_stream", "h2d_kernel"):
        fx, res = headline_host_inputs(opts)
        check_headline_host(fx, res)
        _, want_res = cached("headline_host_default", lambda: headline_host_inputs({}))
        for a, b in zip(res, want_res):
            for k in range(len(a)):
                if isinstance(a[k], dict):
                    assert_same(a[k], b[k], (name, value, k))
                else:
                    assert a[k] == b[k]


def test_depth_option_sets_the_lanes_of_new_handles():
    """depth (a new handle's lanes): with depth = 16, sixteen device batches are in flight at once and a
    seventeenth is refused; with depth = 1 the second is refused."""
    pr = tp.synth_problem(4343, 300, 0.8, 0.01)
    mem = HipBuffers()
    a, b = mem.device(np.ascontiguousarray(pr["src"].T)), mem.device(np.ascontiguousarray(pr["dst"].T))
    off, nn = np.zeros(1, dtype=np.int64), np.array([300], dtype=np.int32)
    want = None
    for depth in (16, 1):
        with options({"depth": depth}):
            s = make_solver(**bench_params())
            tickets = [s.submit_batch(a, b, off, nn) for _ in range(depth)]
            with pytest.raises(tp.TeaserHipError):
                s.submit_batch(a, b, off, nn)
            for t in tickets:
                s.wait(t)
                r = result(s)
                want = want or r
                assert_same(r, want, depth)
            s.close()
    mem.free()
