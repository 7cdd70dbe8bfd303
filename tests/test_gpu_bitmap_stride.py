"""GPU tests of the bitmap arena's 64-byte row stride (csrc/internal.h: bm_stride).  A problem of n vertices has
W = ceil(n / 64) words per row; in the device arena its rows lie bm_stride(W) = W rounded up to a multiple of 8 words
apart, the words W .. stride - 1 of a row are padding and zero on every route that fills a bitmap, and the public
layout (getInlierGraphBitmap) stays dense.  Sizes: one vertex; the last bit of a word, a full word, one bit more (63,
64, 65); the last row of a full stride, a full stride and one word more (449, 512, 513: W = 8, 8, 9); two strides plus a
word (1025: W = 17); and a batch that mixes padded and unpadded problems.  Routes: the default one (matrix-core K1,
upper triangle + mirror), deg_closure = 0 (matrix-core K1, full store) and k1_fp64 = 1."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

from oracle import oracle
from test_gpu_route_switches import make_solver, options, oracle_params, result
from test_gpu_upper_triangle import check_graph, check_solution, exact_params

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")
NB = 0.01
ROUTES = {"default": {}, "full_store": {"deg_closure": 0}, "fp64": {"k1_fp64": 1}}
SIZES = [1, 63, 64, 65, 449, 512, 513, 1025]
MIXED = [513, 64, 1000, 449]
# GPU pose against the oracle's: the bound smoke() holds the same comparison to
POSE_TOL = 1e-4


def stride(n):
    return ((n + 63) // 64 + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def reference(n, kind="synth"):
    """(src, dst, oracle solution, oracle bitmap), computed once per size"""
    if kind == "rigid" or n < 8:  # an exact rigid motion: every pair is consistent, every row all ones
        rng = np.random.default_rng(20261100 + n)
        src = rng.uniform(-1.0, 1.0, size=(3, n))
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        dst = q @ src + np.array([[0.3], [-0.2], [0.1]])
    else:
        pr = tp.synth_problem(20261000 + n, n, 0.8, NB)
        src, dst = pr["src"], pr["dst"]
    src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    sol = oracle.solve(src, dst, **oracle_params(exact_params()))
    _, bm = oracle.inlier_bitmap(src, dst, NB, 1.0, False)
    return src, dst, sol, bm


def check_pose(s, b, sol, what):
    r = s.raw_solution(b)
    assert bool(r.valid) == bool(sol["valid"]), what
    if not sol["valid"]:
        return
    assert s.getRotationInliers(b) == sol["rotation_inliers"].tolist(), what
    assert s.getTranslationInliers(b) == sol["translation_inliers"].tolist(), what
    R = np.array(r.rotation[:], dtype=np.float64).reshape(3, 3)
    assert np.linalg.norm(R - sol["rotation"]) < POSE_TOL, what
    assert np.linalg.norm(np.array(r.translation[:], dtype=np.float64) - np.asarray(sol["translation"]).ravel()) < POSE_TOL, what


def raw_rows(s, b, n):
    """the problem's rows as the arena holds them: [n, stride] words"""
    ln, st = ctypes.c_int64(0), ctypes.c_int32(0)
    fn = s._lib.teaser_hip_get_inlier_graph_rows
    s._check(fn(s._h, b, None, ctypes.byref(ln), ctypes.byref(st)))
    assert st.value == stride(n) and ln.value == n * st.value
    buf = np.zeros(max(ln.value, 1), dtype=np.uint64)
    s._check(fn(s._h, b, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(ln), ctypes.byref(st)))
    return buf[:ln.value].reshape(n, st.value)


def check_problem(s, b, n, sol, bm, what):
    check_solution(result(s, b), sol, what)
    check_pose(s, b, sol, what)
    check_graph(s, b, n, bm)  # the dense bitmap, bit for bit, and the degrees
    rows = raw_rows(s, b, n)  # (behind the getter: both halves are in place)
    W = (n + 63) // 64
    assert (rows[:, :W] == bm).all(), what
    assert not rows[:, W:].any(), what


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("n", SIZES)
def test_stride_edges(n, route):
    src, dst, sol, bm = reference(n)
    with options(ROUTES[route]):
        s = make_solver(**exact_params())
        s.solve(src, dst)
        check_problem(s, 0, n, sol, bm, (n, route))
        s.close()


@pytest.mark.parametrize("route", list(ROUTES))
def test_mixed_batch(route):
    refs = [reference(n) for n in MIXED]
    with options(ROUTES[route]):
        s = make_solver(**exact_params())
        s.solve_batch([r[0] for r in refs], [r[1] for r in refs])
        for b, (n, (_, _, sol, bm)) in enumerate(zip(MIXED, refs)):
            check_problem(s, b, n, sol, bm, (n, route))
        s.close()


@pytest.mark.parametrize("route", list(ROUTES))
def test_stale_padding(route):
    """one handle: a batch of all-ones rows at n = 1000 (stride 16), then n = 449 (stride 8, no padding), then n = 513
    (9 words on a stride of 16: its padding lies where the first two solves left ones).  The later results equal a fresh
    handle's, and the padding of every row is zero."""
    first = reference(1000, "rigid")
    assert oracle.bitmap_to_dense(first[3], 1000).sum() == 1000 * 999
    with options(ROUTES[route]):
        s = make_solver(**exact_params())
        s.solve_batch([first[0], first[0]], [first[1], first[1]])
        for n in (449, 513):
            src, dst, sol, bm = reference(n)
            s.solve_batch([src, src], [dst, dst])
            got = [result(s, b) for b in range(2)]
            rows = [raw_rows(s, b, n) for b in range(2)]  # (before the getter: as the solve left the arena)
            W = (n + 63) // 64
            for b in range(2):
                assert not rows[b][:, W:].any(), (n, route, b)
            fresh = make_solver(**exact_params())
            fresh.solve_batch([src, src], [dst, dst])
            want = [result(fresh, b) for b in range(2)]
            fresh.close()
            assert got == want, (n, route)
            for b in range(2):
                check_problem(s, b, n, sol, bm, (n, route, b))
        s.close()


def test_supplied_graph_of_513_vertices():
    """teaser_hip_max_clique: the caller's dense rows (9 words) are laid out on the arena's stride (16)"""
    n = 513
    _, _, _, bm = reference(n)
    o = oracle.max_clique(bm, n)
    for opts in ({}, {"deg_closure": 0}):
        with options(opts):
            s = make_solver(**exact_params())
            rigid = reference(1000, "rigid")
            s.solve(rigid[0], rigid[1])  # (ones where the supplied graph's padding will lie)
            c, _ = s.maxClique(bm, n)
            s.close()
        assert len(c) == len(o["clique"]), opts
        if o["unique"]:
            assert c == o["clique"].tolist(), opts
        sub = oracle.bitmap_to_dense(bm, n)[np.ix_(c, c)]
        assert (sub | np.eye(len(c), dtype=bool)).all(), opts
