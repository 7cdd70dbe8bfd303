"""GPU tests of the no-store route's degrees and of its open-only rebuild (csrc/kernels_graph.hip:
tim_graph_mfma3_kernel with NS = kK1NoStore and kK1Rebuild, k1_rebuild_find_open).  K1 stores no row there, so the
degrees are all that is left of a wave's off-diagonal column tiles, and the rows of the problems the closure leaves open
come back from a rebuild whose grid is one problem's blocks x 2 slots, the open problems found by scanning the states.

Every case solves on a handle whose previous batch the closure decided, asserts that the solve under test took the
no-store route, compares getDegrees and the rebuilt bitmap bit for bit with the oracle's, and the answer with the
deg_closure = 0 route of the same process.  Complete graphs (exact rigid motions) drive every row's count to its
maximum over every strip of column tiles a wave walks."""
import pytest

from test_gpu_k1_no_store import NONE, graph_route, warmed_solver
from test_gpu_route_switches import result
from test_gpu_upper_triangle import (CLOSED, NB, assert_same_answer, check_graph, check_solution, full_store_route,
                                     reference)

pytestmark = pytest.mark.gpu

STRIP = 8  # column tiles of a wave's strip: kMfmaColTiles * kK1Chunks (kernels_graph.hip)


def solve_no_store(batch):
    """the batch behind a closed batch of the same width on one handle -> the results; graph, degrees, answer checked"""
    k = len(batch)
    warm = reference(("synth90", 640, NB))
    s = warmed_solver()
    if k > 1:  # (warmed_solver closed a batch of one: the batch in front of the one under test has its width)
        s.solve_batch([warm[0]] * k, [warm[1]] * k)
        assert all(result(s, b)["uncoloured"] in CLOSED for b in range(k))
    s.solve_batch([p[0] for p in batch], [p[1] for p in batch])
    assert graph_route(s)[0] == NONE
    got = [result(s, b) for b in range(k)]
    for b, (src, dst, sol, bm) in enumerate(batch):
        check_solution(got[b], sol, b)
        check_graph(s, b, src.shape[1], bm)
    assert graph_route(s)[0] == NONE
    s.close()
    want = full_store_route([p[0] for p in batch], [p[1] for p in batch])
    for b, (src, dst, sol, bm) in enumerate(batch):
        assert_same_answer(got[b], want[b], b, content=sol["clique_unique"])
    return got


@pytest.mark.parametrize("n", sorted({65, 64 * 8 + 1, 64 * STRIP + 1, 64 * STRIP + 65}))
def test_complete_graph_drives_every_counter_to_its_maximum(n):
    """one off-diagonal tile (65); one full chunk (513); the full strip (64 STRIP + 1: the first row tile's wave counts
    STRIP tiles behind its diagonal one in two blocks, every other strip ends at the last tile of one column); a strip
    boundary crossed (64 STRIP + 65)"""
    assert n <= 2177
    src, dst, sol, bm = reference(("rigid", n, NB))
    assert len(sol["max_clique"]) == n
    got = solve_no_store([(src, dst, sol, bm)])[0]
    assert got["size"] == n and got["edges"] == n * (n - 1) // 2


@pytest.mark.parametrize("n", sorted({129, 577, 64 * STRIP + 1}))
def test_synthetic_problems_with_ragged_last_tiles(n):
    """two tiles, the last of one column (129); a ragged last tile behind a chunk edge (577); the last tile of one
    column behind a full strip (64 STRIP + 1)"""
    solve_no_store([reference(("synth80", n, NB))])


def test_two_problems_with_different_tile_counts_in_one_batch():
    """513 and 1025 points: the grid is the larger problem's, the smaller one's blocks beyond its tiles leave early, and
    its last column tile (one column) is not the batch's last"""
    solve_no_store([reference(("synth80", 513, NB)), reference(("synth80", 1025, NB))])


OPEN_LAYOUTS = {"none": "ccccc", "first": "occcc", "last": "cccco", "first_adjacent_last": "oocco"}


@pytest.mark.parametrize("layout", sorted(OPEN_LAYOUTS))
def test_open_only_rebuild_finds_its_problems(layout):
    """the open-only rebuild runs on a grid of one problem's blocks x 2 slots and finds the problems the closure left
    open by scanning the batch's states: none; one, first or last in the batch; three (the first two adjacent, one
    last), so that slot 0 serves a second problem.  Open = two unrelated clouds.  `rebuilt` counts the open problems
    before any getter is called, and every problem's graph, degrees and answer are the oracle's.  (That the rows of the
    closed problems stay untouched cannot be seen through the API: every row getter first rebuilds the whole batch.)"""
    closed, opened = reference(("synth90", 640, NB)), reference(("outliers", 600, NB))
    batch = [opened if c == "o" else closed for c in OPEN_LAYOUTS[layout]]
    k, n_open = len(batch), OPEN_LAYOUTS[layout].count("o")
    s = warmed_solver()
    s.solve_batch([closed[0]] * k, [closed[1]] * k)
    assert all(result(s, b)["uncoloured"] in CLOSED for b in range(k))
    s.solve_batch([p[0] for p in batch], [p[1] for p in batch])
    assert graph_route(s) == (NONE, n_open)
    got = [result(s, b) for b in range(k)]
    for b, (src, dst, sol, bm) in enumerate(batch):
        assert (got[b]["uncoloured"] in CLOSED) == (OPEN_LAYOUTS[layout][b] == "c"), b
        check_solution(got[b], sol, (layout, b))
    assert graph_route(s) == (NONE, n_open)
    for b in reversed(range(k)):
        check_graph(s, b, batch[b][0].shape[1], batch[b][3])
    assert graph_route(s) == (NONE, n_open + k)
    s.close()
    want = full_store_route([p[0] for p in batch], [p[1] for p in batch])
    for b, (src, dst, sol, bm) in enumerate(batch):
        assert_same_answer(got[b], want[b], (layout, b), content=sol["clique_unique"])
