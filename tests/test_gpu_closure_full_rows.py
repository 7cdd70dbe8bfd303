"""GPU tests of the three-launch degree closure behind a K1 that stores no row (csrc/kernels_heuristic.hip:
degree_closure_order_kernel staging R's points in rank order, degree_closure_verdict_kernel<true> computing H from full
rows by csrc/closure_h.h; csrc/kernels_graph.hip: tim_closure_pairs_kernel writing both words of every block).

Every case is solved on the no-store route -- a second solve on a handle whose first batch the closure decided,
teaser_hip_get_graph_route = 2 -- and held byte for byte to the same problems on the deg_closure = 0 route and on a
fresh handle's upper-triangle route (order, rows, symmetrise, verdict from the bitmap): clique, degrees, edge count,
the closure's verdict, R, t and the inlier lists; and to the oracle (solution, graph, degrees)."""
import ctypes

import numpy as np
import pytest

from test_gpu_k1_no_store import NONE, UPPER, graph_route, warmed_solver
from test_gpu_route_switches import make_solver, options, result
from test_gpu_upper_triangle import (CLOSED, NB, assert_same_answer, check_graph, check_solution, exact_params,
                                     full_store_route, reference)
from util import HipBuffers

pytestmark = pytest.mark.gpu

CORE_CAP = 2048  # kCoreCap (csrc/internal.h)
ANSWER = ("valid", "status", "size", "edges", "uncoloured", "scale", "R", "t", "clique", "rot", "trans")


def upper_route(batch):
    """a fresh handle's first solve: K1 stores the upper triangle, the closure runs its four launches"""
    s = make_solver(**exact_params())
    s.solve_batch([p[0] for p in batch], [p[1] for p in batch])
    assert graph_route(s)[0] == UPPER
    out = [(result(s, b), s.getDegrees(b).copy()) for b in range(len(batch))]
    s.close()
    return out


def solve_three_launch(batch):
    """the batch behind a closed batch of the same width on one handle -> its results, every comparison made"""
    k = len(batch)
    warm = reference(("synth90", 640, NB))
    s = warmed_solver()
    if k > 1:
        s.solve_batch([warm[0]] * k, [warm[1]] * k)
        assert all(result(s, b)["uncoloured"] in CLOSED for b in range(k))
    s.solve_batch([p[0] for p in batch], [p[1] for p in batch])
    assert graph_route(s)[0] == NONE
    got = [result(s, b) for b in range(k)]
    deg = [s.getDegrees(b).copy() for b in range(k)]
    for b, (src, dst, sol, bm) in enumerate(batch):
        check_solution(got[b], sol, b)
        check_graph(s, b, src.shape[1], bm)
    s.close()
    full = full_store_route([p[0] for p in batch], [p[1] for p in batch])
    upper = upper_route(batch)
    for b, (src, dst, sol, bm) in enumerate(batch):
        assert_same_answer(got[b], full[b], ("deg_closure = 0", b), content=sol["clique_unique"])
        diff = [key for key in ANSWER if got[b][key] != upper[b][0][key]]
        assert not diff, ("upper-triangle route", b, diff)
        assert (deg[b] == upper[b][1]).all(), b
    return got


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 127, 128, 129, 513, 2048, 2049])
def test_complete_graphs(n):
    """m = n: every block edge of the pair kernel and of the H walk; at 2049 R exceeds kCoreCap, the closure declines
    and the open-only rebuild and the heuristic chain run"""
    src, dst, sol, bm = reference(("rigid", n, NB))
    assert len(sol["max_clique"]) == n
    got = solve_three_launch([(src, dst, sol, bm)])[0]
    assert got["size"] == n and got["edges"] == n * (n - 1) // 2
    if 63 <= n <= CORE_CAP:
        assert got["uncoloured"] in CLOSED  # (the three launches decided it)
    if n > CORE_CAP:
        assert got["uncoloured"] not in CLOSED


@pytest.mark.parametrize("n", [129, 513, 577])
def test_candidate_set_is_a_strict_subset_in_permuted_order(n):
    """R is a strict subset of the vertices and the ranks permute them: a wrong gather of the staged points shows"""
    got = solve_three_launch([reference(("synth80", n, NB))])[0]
    assert got["uncoloured"] in CLOSED and got["size"] < n


def test_mixed_batch_with_a_single_point_and_an_open_problem():
    batch = [reference(("rigid", 1, NB)), reference(("synth80", 65, NB)), reference(("synth80", 513, NB)),
             reference(("synth80", 1025, NB)), reference(("outliers", 600, NB))]
    got = solve_three_launch(batch)
    assert got[2]["uncoloured"] in CLOSED and got[3]["uncoloured"] in CLOSED and got[4]["uncoloured"] not in CLOSED


@pytest.mark.parametrize("wgs", [1, 16, 64])
def test_every_grid_of_the_pair_kernel(wgs):
    with options({"deg_closure_wgs": wgs}):
        got = solve_three_launch([reference(("synth80", 513, NB))])[0]
    assert got["uncoloured"] in CLOSED


def test_two_lanes_with_inputs_overwritten_before_the_getters():
    """submit / wait at depth 2, each lane warmed by a closed batch; after wait every input double becomes a NaN, then
    the getters are called: the staged points are read inside the solve only"""
    names = [[("synth90", 640, NB)] * 2, [("synth90", 640, NB)] * 2,
             [("synth80", 513, NB), ("rigid", 129, NB)], [("synth80", 577, NB), ("synth80", 129, NB)]]
    refs = [[reference(key) for key in batch] for batch in names]
    sync = []
    s0 = make_solver(**exact_params())
    for batch in refs:
        s0.solve_batch([p[0] for p in batch], [p[1] for p in batch])
        sync.append([result(s0, b) for b in range(len(batch))])
    s0.close()
    mem = HipBuffers()
    s = make_solver(**exact_params())
    s.set_pipeline_depth(2)
    tickets, inputs = [], []
    for batch in refs:
        src = np.ascontiguousarray(np.concatenate([p[0].T for p in batch], axis=0))
        dst = np.ascontiguousarray(np.concatenate([p[1].T for p in batch], axis=0))
        nn = np.array([p[0].shape[1] for p in batch], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(nn)[:-1]]).astype(np.int64)
        inputs.append((mem.device(src), mem.device(dst), src.nbytes))
        tickets.append(s.submit_batch(inputs[-1][0], inputs[-1][1], off, nn))
        if len(tickets) == 2:  # both lanes have finished a closed batch before the batches under test are submitted
            for t in tickets:
                s.wait(t)
    for k in (2, 3):
        s.wait(tickets[k])
        assert graph_route(s)[0] == NONE, k
        for ptr in inputs[k][:2]:
            assert mem.hip.hipMemset(ctypes.c_void_p(ptr), 0xff, ctypes.c_size_t(inputs[k][2])) == 0
        assert mem.hip.hipDeviceSynchronize() == 0
        for b, (src, dst, sol, bm) in enumerate(refs[k]):
            r = result(s, b)
            assert r["uncoloured"] in CLOSED, (k, b)
            check_solution(r, sol, (k, b))
            diff = [key for key in ANSWER if r[key] != sync[k][b][key]]
            assert not diff, (k, b, diff)
            check_graph(s, b, src.shape[1], bm)
    s.close()
    mem.free()
