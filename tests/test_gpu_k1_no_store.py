"""GPU tests of the no-store route of K1 (csrc/kernels_graph.hip: tim_graph_mfma3_kernel with NS = kK1NoStore and
kK1Rebuild, tim_fixup_group_kernel<true>, tim_fixup_replay_kernel, tim_closure_pairs_kernel;
csrc/solver.hip: the routing, enqueue_graph_rebuild, the getters).  Once a handle has finished a batch the degree
closure decided (almost) entirely, its next K1 stores no row: the closure evaluates the pairs of its candidate set from
the points, the fix-up records its answers in the worklist items, and the rows are rebuilt from the handle's own arenas
for the problems the closure leaves open and for the graph getters.

Every case first solves a problem the closure decides on the same handle, asserts through teaser_hip_get_graph_route
that the solve under test took the no-store route, and compares the result with the oracle and with the
deg_closure = 0 route (full store) of the same process: solution, clique where unique, inlier lists, degrees and the
dense bitmap bit for bit."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

from fixup_row_tiles_model import ENGINEERED_BETA, REGION_ITEMS, WAVE_BUFFER, engineered_1100, items_per_cell, min_abs_d
from oracle import oracle
from test_gpu_bitmap_stride import raw_rows
from test_gpu_k1_f16 import admitted
from test_gpu_route_switches import make_solver, options, oracle_params, result
from test_gpu_upper_triangle import (CLOSED, NB, assert_same_answer, check_graph, check_solution, cols, declined,
                                     exact_params, full_store_route, reference)
from test_k1_f16_band_model import adversarial
from util import HipBuffers

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")
FULL, UPPER, NONE = 0, 1, 2


def graph_route(s, b=0):
    """(how the last solve's K1 stored the graph, problems rebuilt since)"""
    route, rebuilt = ctypes.c_int32(-1), ctypes.c_int64(-1)
    s._check(s._lib.teaser_hip_get_graph_route(s._h, b, ctypes.byref(route), ctypes.byref(rebuilt)))
    return route.value, rebuilt.value


def closed_problem():
    return reference(("synth90", 640, NB))


def warmed_solver(nb=NB, **kw):
    """a handle whose previous batch the closure decided entirely: its next closure-route solve stores no row.  (At
    another noise bound than the synthetic problem's the warm-up is an exact rigid motion: a complete graph.)"""
    src, dst, sol, _ = closed_problem() if nb == NB else reference(("rigid", 640, NB))
    s = make_solver(**exact_params(nb, **kw))
    s.solve(src, dst)
    r = result(s)
    assert r["uncoloured"] in CLOSED and r["size"] == len(sol["max_clique"])
    assert graph_route(s) == (UPPER, 0)  # a fresh handle's first solve: the storing route
    return s


@pytest.mark.parametrize("n", [64, 65, 257, 512, 513, 577, 1025, 2049])
def test_tile_and_chunk_edges(n):
    """the diagonal tile alone (64); one off-diagonal block (65); two row groups (257); chunk edges and their padding
    (512, 513); a ragged last tile (577); more than one chunk pair (1025, 2049)"""
    src, dst, sol, bm = reference(("synth80", n, NB))
    s = warmed_solver()
    s.solve(src, dst)
    assert graph_route(s)[0] == NONE
    r = result(s)
    check_solution(r, sol, n)
    assert s.getRotationInliers() == sol["rotation_inliers"].tolist() or not sol["clique_unique"]
    assert s.getTranslationInliers() == sol["translation_inliers"].tolist() or not sol["clique_unique"]
    open_now = 0 if r["uncoloured"] in CLOSED else 1
    assert graph_route(s) == (NONE, open_now)
    check_graph(s, 0, n, bm)  # (twice: the second call finds the rows in place)
    assert graph_route(s) == (NONE, open_now + 1)  # ... rebuilt once
    rows = raw_rows(s, 0, n)
    W = (n + 63) // 64
    assert (rows[:, :W] == bm).all() and not rows[:, W:].any()
    s.close()
    want = full_store_route([src], [dst])[0]
    assert_same_answer(r, want, n, content=sol["clique_unique"])


@pytest.mark.parametrize("skip_closed", [0, 1])
def test_closure_declines_and_the_rebuild_feeds_the_stages_behind_it(skip_closed):
    """two unrelated clouds behind a closed batch: greedy, peel and the exact search read rows the head of the
    heuristic stage has rebuilt -- enqueued behind the closure, or (heu_skip_closed = 1) by the finish half"""
    n, src, dst, sol, bm, want = declined()
    with options({"heu_skip_closed": skip_closed}):
        s = warmed_solver()
        s.solve(src, dst)
        assert graph_route(s) == (NONE, 1)
        r = result(s)
        assert r["uncoloured"] not in CLOSED
        check_solution(r, sol, ("declined", skip_closed))
        assert_same_answer(r, want, ("declined", skip_closed), content=sol["clique_unique"])
        check_graph(s, 0, n, bm)
        s.close()


def test_mixed_batch_of_closed_open_and_fp64_body_problems():
    """the three routes in one launch (after test_gpu_upper_triangle.py), behind a closed batch of the same width"""
    nb, f = 1e-7, 2.0 ** -13
    a = tp.synth_problem(20260501, 640, 0.5, nb / f)
    rng = np.random.default_rng(20260502)
    c = tp.synth_problem(20260503, 700, 0.5, nb)
    srcs = [np.ascontiguousarray(a["src"] * f), np.ascontiguousarray(rng.uniform(-1.0, 1.0, size=(3, 190)) * f), c["src"]]
    dsts = [np.ascontiguousarray(a["dst"] * f), np.ascontiguousarray(rng.uniform(-1.0, 1.0, size=(3, 190)) * f), c["dst"]]
    assert admitted(srcs[0], dsts[0], nb) and admitted(srcs[1], dsts[1], nb) and not admitted(srcs[2], dsts[2], nb)
    s = make_solver(**exact_params(nb))
    s.solve_batch([srcs[0]] * 3, [dsts[0]] * 3)
    assert all(result(s, b)["uncoloured"] in CLOSED for b in range(3))
    s.solve_batch(srcs, dsts)
    assert graph_route(s)[0] == NONE
    got = [result(s, b) for b in range(3)]
    assert got[0]["uncoloured"] in CLOSED and got[1]["uncoloured"] not in CLOSED
    want = full_store_route(srcs, dsts, nb)
    for b in range(3):
        sol = oracle.solve(srcs[b], dsts[b], **oracle_params(exact_params(nb)))
        _, bm = oracle.inlier_bitmap(srcs[b], dsts[b], nb, 1.0, False)
        check_solution(got[b], sol, b)
        assert_same_answer(got[b], want[b], b, content=sol["clique_unique"])
        check_graph(s, b, srcs[b].shape[1], bm)
    s.close()


def test_route_sequence_follows_the_previous_batch():
    """closed -> open -> closed -> closed on one handle: upper (fresh), none, upper (the open batch broke the rule),
    none; every result equals a fresh handle's"""
    csrc, cdst, csol, cbm = closed_problem()
    n, osrc, odst, osol, obm, _ = declined()
    seq = [(csrc, cdst, csol, cbm, UPPER), (osrc, odst, osol, obm, NONE), (csrc, cdst, csol, cbm, UPPER),
           (csrc, cdst, csol, cbm, NONE)]
    fresh = {}
    s = make_solver(**exact_params())
    for k, (src, dst, sol, bm, route) in enumerate(seq):
        s.solve(src, dst)
        assert graph_route(s)[0] == route, k
        r = result(s)
        check_solution(r, sol, k)
        if id(src) not in fresh:
            f = make_solver(**exact_params())
            f.solve(src, dst)
            fresh[id(src)] = result(f)
            f.close()
        assert r == fresh[id(src)], k
        check_graph(s, 0, src.shape[1], bm)
    s.close()


def test_batches_of_other_widths_and_sizes_than_the_one_before():
    """one problem of 640 points, then three of 257 / 1025 / 640, then one of 2049, all but the first without stores: the
    rebuilds take the batch, its largest problem, its tile total and its worklist capacity from the CURRENT solve"""
    s = warmed_solver()
    wide = [reference(k) for k in (("synth80", 257, NB), ("synth80", 1025, NB), ("synth90", 640, NB))]
    for batch in (wide, [reference(("rigid", 640, NB))], [reference(("synth80", 2049, NB))]):
        s.solve_batch([p[0] for p in batch], [p[1] for p in batch])
        got = [result(s, b) for b in range(len(batch))]
        n_open = sum(r["uncoloured"] not in CLOSED for r in got)
        assert graph_route(s) == (NONE, n_open)
        for b in reversed(range(len(batch))):  # (the getter's rebuild is triggered through the LAST problem)
            src, dst, sol, bm = batch[b]
            check_solution(got[b], sol, b)
            check_graph(s, b, src.shape[1], bm)
        assert graph_route(s) == (NONE, n_open + len(batch))
        if n_open:  # (a problem the closure left open puts the next batch on the storing route: close one in between)
            s.solve(*closed_problem()[:2])
            assert result(s)["uncoloured"] in CLOSED
    s.close()


def test_stale_arena_is_fully_redefined_by_the_getters_rebuild():
    """all-ones rows at n = 1000 first (it also warms the route: a rigid motion is closed), then n = 449 and n = 513 on
    the no-store route: the rebuild defines every word and every padding word"""
    first = reference(("rigid", 1000, NB))
    assert oracle.bitmap_to_dense(first[3], 1000).sum() == 1000 * 999
    s = make_solver(**exact_params())
    s.solve_batch([first[0], first[0]], [first[1], first[1]])
    assert all(result(s, b)["uncoloured"] in CLOSED for b in range(2))
    for n in (449, 513):
        src, dst, sol, bm = reference(("synth80", n, NB))
        s.solve_batch([src, src], [dst, dst])
        assert graph_route(s)[0] == NONE, n
        W = (n + 63) // 64
        for b in range(2):
            check_solution(result(s, b), sol, (n, b))
            rows = raw_rows(s, b, n)
            assert (rows[:, :W] == bm).all() and not rows[:, W:].any(), (n, b)
            check_graph(s, b, n, bm)
    s.close()


def no_store_fixup_case(src, dst, beta, need_overflow):
    """src, dst [n, 3] boundary-engineered pairs: the graph after write-back and replay of the items, those of the
    counted segment included where the CPU band model says a region holds twice its 63 items.  No K1 wave may stage more
    than it can hold, with a factor of two on the band: such a batch reruns on the all-FP64 K1, off the route under
    test (the route assertion would catch it)."""
    mins, C, adm = min_abs_d(src, dst, beta)
    assert adm
    cnt = items_per_cell(mins, C)
    if need_overflow:
        assert cnt.max() >= 2 * REGION_ITEMS  # more items than a region holds: the counted segment is in use
    assert 2 * cnt.max() <= WAVE_BUFFER, cnt.max()
    # (The oracle's full solve of these clouds -- every point an inlier displaced by about beta: a dense graph with no
    # clique to speak of -- does not end within minutes on the CPU, so its graph and degrees are the reference, and the
    # solve's answer is compared with the deg_closure = 0 route's: the edge count always, and everything that does not
    # depend on which maximum clique was found first wherever neither search hit its time limit.)
    s = warmed_solver(beta / 2, max_clique_time_limit=0.5)
    s.solve(cols(src), cols(dst))
    assert graph_route(s)[0] == NONE
    r = result(s)
    _, bm = oracle.inlier_bitmap(cols(src), cols(dst), beta / 2, 1.0, False)
    check_graph(s, 0, len(src), bm)
    s.close()
    want = full_store_route([cols(src)], [cols(dst)], beta / 2, max_clique_time_limit=0.5)[0]
    assert r["edges"] == want["edges"]
    if r["status"] == 0 and want["status"] == 0:
        assert_same_answer(r, want, "fix-up case", content=False)


def test_item_overflow_into_the_counted_segment():
    """the engineered-beta input of test_gpu_fixup_row_tiles.py: regions with more than 63 items, a row tile with two
    queue rounds, a row tile with no item"""
    src, dst = engineered_1100(101)
    no_store_fixup_case(src, dst, ENGINEERED_BETA, True)


def test_adversarial_band_with_many_flipped_bits():
    src, dst = adversarial(np.random.default_rng(32), 1024, 1.0, 2 * NB)
    no_store_fixup_case(src, dst, 2 * NB, False)


def test_two_lanes_and_a_getter_behind_overwritten_inputs():
    """submit_batch / wait on device-resident inputs, two lanes alternating, each lane warmed by a closed batch; results
    equal the synchronous call's.  After wait the input arrays are overwritten and THEN the bitmap getter is called:
    it still returns the oracle's graph, because the rebuild reads nothing of the caller's."""
    names = [[("synth90", 640, NB)], [("synth90", 640, NB)],
             [("synth80", 577, NB), ("outliers", 600, NB)], [("synth80", 257, NB), ("rigid", 640, NB)]]
    refs = [[reference(k) for k in batch] for batch in names]
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
        batch = refs[k]
        s.wait(tickets[k])
        assert graph_route(s)[0] == NONE, k
        for ptr in inputs[k][:2]:  # every input double becomes a NaN
            assert mem.hip.hipMemset(ctypes.c_void_p(ptr), 0xff, ctypes.c_size_t(inputs[k][2])) == 0
        assert mem.hip.hipDeviceSynchronize() == 0
        for b, (src, dst, sol, bm) in enumerate(batch):
            r = result(s, b)
            check_solution(r, sol, (k, b))
            assert_same_answer(r, sync[k][b], (k, b), content=sol["clique_unique"])
            check_graph(s, b, src.shape[1], bm)
    s.close()
    mem.free()
