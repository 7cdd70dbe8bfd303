"""GPU tests of the upper-triangle route of K1 (csrc/kernels_graph.hip: tim_graph_mfma3_kernel with LOWER = false,
tim_mirror_lower_kernel; csrc/fixup_item.h; csrc/kernels_heuristic.hip: the degree closure's pick rule and its
symmetrise launch; csrc/solver.hip: the routing).  With PMC_EXACT and default options K1 stores the bitmap's upper
triangle only, the fix-up takes an item's provisional bits from the item, the degree closure reads a row from word
r / 64 on, and the lower triangle is rebuilt by the mirror kernel for the problems the closure leaves open and for the
bitmap getter.  Everything is compared with the oracle and with the deg_closure = 0 route (full store) of the same
process."""
import functools
import importlib

import numpy as np
import pytest

from fixup_row_tiles_model import ENGINEERED_BETA, ROUND_ITEMS, WAVE_BUFFER, items_per_cell, min_abs_d
from oracle import oracle
from test_gpu_k1_f16 import admitted
from test_gpu_route_switches import bench_params, make_solver, options, oracle_params, result
from test_k1_f16_band_model import adversarial
from util import HipBuffers

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")
NB = 0.01
CLOSED = (-2, -3)  # colour_uncoloured of a problem the degree closure decided (-3: a maximum clique that is not unique)


def exact_params(nb=NB, **kw):
    return bench_params(noise_bound=nb, inlier_selection_mode=tp.InlierSelectionMode.PMC_EXACT, **kw)


def cols(a):
    return np.ascontiguousarray(a.T)  # [n, 3] -> the solver's [3, n]


@functools.lru_cache(maxsize=None)
def reference(key):
    """(src, dst, oracle solution, oracle bitmap) of a named problem, computed once"""
    kind, n, nb = key
    if kind == "synth80":
        pr = tp.synth_problem(20260100 + n, n, 0.8, nb)
        src, dst = pr["src"], pr["dst"]
    elif kind == "synth90":
        pr = tp.synth_problem(20260200 + n, n, 0.9, nb)
        src, dst = pr["src"], pr["dst"]
    elif kind == "rigid":  # an exact rigid motion: every pair is consistent
        rng = np.random.default_rng(20260300 + n)
        src = rng.uniform(-1.0, 1.0, size=(3, n))
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        dst = q @ src + np.array([[0.3], [-0.2], [0.1]])
    elif kind == "outliers":  # two unrelated clouds
        rng = np.random.default_rng(20260400 + n)
        src, dst = rng.uniform(-1.0, 1.0, size=(3, n)), rng.uniform(-1.0, 1.0, size=(3, n))
    else:
        raise KeyError(kind)
    src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    sol = oracle.solve(src, dst, **oracle_params(exact_params(nb)))
    _, bm = oracle.inlier_bitmap(src, dst, nb, 1.0, False)
    return src, dst, sol, bm


def check_graph(s, b, n, bm):
    got = s.getInlierGraphBitmap(b)
    assert (got == bm).all()
    assert (s.getDegrees(b) == oracle.bitmap_to_dense(bm, n).sum(1)).all()
    assert (s.getInlierGraphBitmap(b) == got).all()  # (the second call finds both halves in place)


def check_solution(r, sol, what):
    assert r["size"] == len(sol["max_clique"]) and r["edges"] == sol["num_edges"] and bool(r["valid"]) == sol["valid"], what
    if sol["clique_unique"]:
        assert list(r["clique"]) == list(sol["max_clique"]), what
    if r["uncoloured"] in CLOSED:  # the closure's verdict on uniqueness is the oracle's
        assert (r["uncoloured"] == -2) == sol["clique_unique"], what


def assert_same_answer(got, want, what, content=True):
    """the answer of a solve, bit for bit -- not how it was reached (heuristic size, exact run, the closure's marker).
    content=False: a maximum clique that is not unique may differ between routes; its size and the edges may not."""
    keys = ["valid", "status", "size", "edges"] + (["scale", "R", "t", "clique", "rot", "trans"] if content else [])
    diff = [k for k in keys if got[k] != want[k]]
    assert not diff, (what, diff, [(got[k], want[k]) for k in diff if k not in ("R", "t", "scale")])


def full_store_route(srcs, dsts, nb=NB, **kw):
    """the same problems with deg_closure = 0: K1 stores both halves, greedy / peel / exact search decide"""
    with options({"deg_closure": 0}):
        s = make_solver(**exact_params(nb, **kw))
        s.solve_batch(srcs, dsts)
        out = [result(s, b) for b in range(len(srcs))]
        s.close()
    return out


@pytest.mark.parametrize("n", [64, 65, 257, 577, 2049])
def test_tile_edges(n):
    """a diagonal tile alone (64); one off-diagonal block (65); two row groups (257); two column chunks with a ragged
    last tile (577); more than one chunk pair (2049)"""
    src, dst, sol, bm = reference(("synth80", n, NB))
    s = make_solver(**exact_params())
    s.solve(src, dst)
    r = result(s)
    check_solution(r, sol, n)
    check_graph(s, 0, n, bm)
    s.close()
    want = full_store_route([src], [dst])[0]
    assert_same_answer(r, want, n, content=sol["clique_unique"])


def test_stale_lower_half_is_never_read():
    """all-ones rows from a first solve lie in the arena's lower triangle when the second, same-n problem is solved: a
    closure that read a word in front of r / 64 would see every early vertex adjacent to every late one"""
    n = 640
    src1, dst1, sol1, bm1 = reference(("rigid", n, NB))
    assert oracle.bitmap_to_dense(bm1, n).sum() == n * (n - 1) and len(sol1["max_clique"]) == n
    src2, dst2, sol2, bm2 = reference(("synth90", n, NB))
    s = make_solver(**exact_params())
    s.solve(src1, dst1)
    r1 = result(s)
    assert r1["uncoloured"] in CLOSED and r1["size"] == n
    s.solve(src2, dst2)
    r2 = result(s)
    assert r2["uncoloured"] in CLOSED  # the closure decided it: its verdict and clique are under test
    check_solution(r2, sol2, "second solve")
    check_graph(s, 0, n, bm2)
    s.close()


@functools.lru_cache(maxsize=None)
def declined():
    n = 600
    src, dst, sol, bm = reference(("outliers", n, NB))
    want = full_store_route([src], [dst])[0]
    return n, src, dst, sol, bm, want


def test_closure_declines_and_the_mirror_feeds_the_stages_behind_it():
    n, src, dst, sol, bm, want = declined()
    s = make_solver(**exact_params())
    s.solve(src, dst)
    r = result(s)
    assert r["uncoloured"] not in CLOSED  # peel, greedy and the exact search ran on this problem's rows
    check_solution(r, sol, "declined")
    assert_same_answer(r, want, "declined", content=sol["clique_unique"])
    check_graph(s, 0, n, bm)
    s.close()


def test_closure_declines_behind_an_all_closed_batch_with_heu_skip_closed():
    """heu_skip_closed = 1: behind a batch the closure decided entirely the heuristic stage is not enqueued; the finish
    half runs it -- mirror first -- for the problem the closure leaves open"""
    n, src, dst, sol, bm, want = declined()
    csrc, cdst, csol, _ = reference(("synth90", 640, NB))
    with options({"heu_skip_closed": 1}):
        s = make_solver(**exact_params())
        s.solve(csrc, cdst)
        rc = result(s)
        assert rc["uncoloured"] in CLOSED
        check_solution(rc, csol, "closed batch")
        s.solve(src, dst)
        r = result(s)
        assert r["uncoloured"] not in CLOSED
        check_solution(r, sol, "declined, heu_skip_closed")
        assert_same_answer(r, want, "declined, heu_skip_closed", content=sol["clique_unique"])
        check_graph(s, 0, n, bm)
        s.close()


def test_mixed_batch_of_closed_open_and_fp64_body_problems():
    """a 10-tile problem, a 3-tile problem the closure leaves open and one that fails the admission test (FP64 body
    inside the launch: both halves stored), after test_gpu_k1_f16.py: beta = 2e-7 is below the filter's resolution on
    a unit cloud, within it on a cloud shrunk by 2^-13"""
    nb, f = 1e-7, 2.0 ** -13
    a = tp.synth_problem(20260501, 640, 0.5, nb / f)
    rng = np.random.default_rng(20260502)
    c = tp.synth_problem(20260503, 700, 0.5, nb)
    srcs = [np.ascontiguousarray(a["src"] * f), np.ascontiguousarray(rng.uniform(-1.0, 1.0, size=(3, 190)) * f), c["src"]]
    dsts = [np.ascontiguousarray(a["dst"] * f), np.ascontiguousarray(rng.uniform(-1.0, 1.0, size=(3, 190)) * f), c["dst"]]
    assert admitted(srcs[0], dsts[0], nb) and admitted(srcs[1], dsts[1], nb) and not admitted(srcs[2], dsts[2], nb)
    s = make_solver(**exact_params(nb))
    s.solve_batch(srcs, dsts)
    got = [result(s, b) for b in range(3)]
    assert got[0]["uncoloured"] in CLOSED and got[1]["uncoloured"] not in CLOSED  # closed and open ones together
    want = full_store_route(srcs, dsts, nb)
    for b in range(3):
        sol = oracle.solve(srcs[b], dsts[b], **oracle_params(exact_params(nb)))
        _, bm = oracle.inlier_bitmap(srcs[b], dsts[b], nb, 1.0, False)
        check_solution(got[b], sol, b)
        assert_same_answer(got[b], want[b], b, content=sol["clique_unique"])
        check_graph(s, b, srcs[b].shape[1], bm)
    s.close()


def fixup_case(src, dst, beta, filter_route, second_round):
    """src, dst [n, 3] boundary-engineered pairs through PMC_EXACT: the CPU band model asserts, with a factor of two on
    the band, that items come from a diagonal and from an off-diagonal tile (and, where asked, that no K1 wave stages
    more items than it can hold -- such a batch is rerun on the all-FP64 K1, which stores both halves: the other cases
    may take that route, arena flag and all -- and that a row tile's queue runs a second round) before the GPU is
    called"""
    mins, C, adm = min_abs_d(src, dst, beta)
    assert adm
    T = mins.shape[0]
    sure = mins <= C / 2
    assert any(sure[I, :, 64 * I:64 * (I + 1)].any() for I in range(T))       # an item of a diagonal tile
    assert any(sure[I, :, 64 * (I + 1):].any() for I in range(T - 1))         # ... of an off-diagonal tile
    cnt = items_per_cell(mins, C)
    if filter_route:
        assert 2 * cnt.max() <= WAVE_BUFFER, cnt.max()
    if second_round:
        assert any(cnt[I].sum() >= 2 * ROUND_ITEMS and (cnt[I] >= 2).sum() >= 2 for I in range(T))
    s = make_solver(**exact_params(beta / 2, max_clique_time_limit=0.5))  # (only the graph is under test)
    s.solve(cols(src), cols(dst))
    _, bm = oracle.inlier_bitmap(cols(src), cols(dst), beta / 2, 1.0, False)
    check_graph(s, 0, len(src), bm)
    s.close()


@pytest.mark.parametrize("scale,nb", [(1.0, 0.01), (250.0, 0.05), (0.02, 1e-4)])
def test_fixup_takes_the_provisional_bits_from_the_items(scale, nb):
    src, dst = adversarial(np.random.default_rng(32), 1024, scale, 2 * nb)
    fixup_case(src, dst, 2 * nb, scale == 1.0, False)


def test_fixup_second_round_of_a_waves_queue():
    src, dst = adversarial(np.random.default_rng(1300), 1300, 1.0, ENGINEERED_BETA)
    fixup_case(src, dst, ENGINEERED_BETA, True, True)


def test_two_batches_in_flight_have_their_own_arenas():
    """submit_batch / wait with two lanes: each lane's arena carries its own flag, so each batch's getter rebuilds its
    own lower triangle; results equal the synchronous solve's"""
    names = [[("synth90", 640, NB), ("outliers", 600, NB)], [("synth80", 257, NB), ("rigid", 640, NB)]]
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
    tickets = []
    for batch in refs:
        src = np.ascontiguousarray(np.concatenate([p[0].T for p in batch], axis=0))
        dst = np.ascontiguousarray(np.concatenate([p[1].T for p in batch], axis=0))
        nn = np.array([p[0].shape[1] for p in batch], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(nn)[:-1]]).astype(np.int64)
        tickets.append(s.submit_batch(mem.device(src), mem.device(dst), off, nn))
    for k, batch in enumerate(refs):
        s.wait(tickets[k])
        for b, (src, dst, sol, bm) in enumerate(batch):
            r = result(s, b)
            check_solution(r, sol, (k, b))
            assert_same_answer(r, sync[k][b], (k, b), content=sol["clique_unique"])
            check_graph(s, b, src.shape[1], bm)
    s.close()
    mem.free()
