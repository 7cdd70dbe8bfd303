"""GPU tests of the fix-up by row tile (csrc/kernels_graph.hip: tim_fixup_group_kernel, csrc/fixup_regions.h): one wave
per 64-row tile walks the tile's regions (one per column chunk of 8 column tiles), queues their items and resolves
them in dense rounds of 64.  Bitmap and degrees equal the oracle's bit for bit at the smallest sizes at which each
path exists; inputs come from the boundary-engineered generator `adversarial`.  Whether an input reaches its regime
is ASSERTED before the GPU is called, from the CPU band model (tests/fixup_row_tiles_model.py) with a factor of two
over the threshold (the model's accumulation order is not the device's) -- a case that missed its regime, or whose
batch took the FP64 rerun, would prove nothing."""
import functools
import importlib

import numpy as np
import pytest

from fixup_row_tiles_model import (ENGINEERED_BETA, REGION_ITEMS, ROUND_ITEMS, WAVE_BUFFER, engineered_1100,
                                   items_per_cell, min_abs_d, n_chunks)
from test_gpu_k1_f16 import admitted, check_problem, k1_only_solver
from test_k1_f16_band_model import adversarial

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")

BETA = 0.02  # (noise bound 0.01) of the plain cases


@functools.lru_cache(maxsize=None)
def plain(n):
    """[n, 3] clouds and the model's item counts per (row tile, column chunk), seeds chosen on the CPU"""
    src, dst = adversarial(np.random.default_rng(200 + n), n, 1.0, BETA)
    mins, C, adm = min_abs_d(src, dst, BETA)
    assert adm
    return src, dst, items_per_cell(mins, C)


@functools.lru_cache(maxsize=None)
def engineered():
    src, dst = engineered_1100(101)
    mins, C, adm = min_abs_d(src, dst, ENGINEERED_BETA)
    assert adm
    return src, dst, items_per_cell(mins, C), items_per_cell(mins, 2 * C)


def cols(a):
    return np.ascontiguousarray(a.T)  # the solver takes [3, n]


def assert_no_wave_overflows(cnt):
    """a K1 wave stages at most 384 items per chunk; beyond that the batch reruns on the FP64 kernel"""
    assert 2 * cnt.max() <= WAVE_BUFFER, cnt.max()


def assert_engineered_regimes():
    _, _, cnt, cnt2 = engineered()
    T, nch = cnt.shape
    assert (T, nch) == (18, 3)
    assert_no_wave_overflows(cnt)
    # a row tile with more than 64 items spread over at least two regions: a second queue round runs
    assert any(cnt[I].sum() >= 2 * ROUND_ITEMS and (cnt[I] >= 2).sum() >= 2 for I in range(T))
    # a region with more than 63 items: the counted segment runs
    assert cnt.max() >= 2 * REGION_ITEMS
    # a row tile with no item, with a factor of two on the band itself
    assert cnt2[5].sum() == 0 and all(cnt[I].sum() > 0 for I in range(T) if I != 5)


def solve_and_check(clouds, nb):
    s = k1_only_solver(nb)
    srcs, dsts = [cols(c[0]) for c in clouds], [cols(c[1]) for c in clouds]
    for a, b in zip(srcs, dsts):
        assert admitted(a, b, nb)
    if len(clouds) == 1:
        s.solve(srcs[0], dsts[0])
    else:
        s.solve_batch(srcs, dsts)
    for p in range(len(clouds)):
        check_problem(s, p, srcs[p], dsts[p], nb)


@pytest.mark.parametrize("n", [65, 130])
def test_one_column_chunk(n):
    """one column chunk: every row tile's only region is the diagonal one; the last row tile is partial"""
    src, dst, cnt = plain(n)
    T = (n + 63) // 64
    assert n_chunks(T) == 1 and n % 64 != 0 and cnt.shape == (T, 1)
    assert cnt.sum() >= 2 and cnt[-1, 0] >= 1  # (items exist, also in the partial tile: 2, 1 at n = 65)
    assert_no_wave_overflows(cnt)
    solve_and_check([(src, dst)], BETA / 2)


@pytest.mark.parametrize("n", [520, 577])
def test_two_column_chunks(n):
    """two column chunks: a row tile merges the regions of two chunks into one queue, the last row tile is partial
    and its only region is the diagonal one, the last row group of K1 has fewer than four row tiles"""
    src, dst, cnt = plain(n)
    T = (n + 63) // 64
    assert n_chunks(T) == 2 and n % 64 != 0 and T % 4 != 0
    assert any((cnt[I] >= 2).all() for I in range(8))      # one queue fed from both chunks
    assert cnt[8:, 0].sum() == 0 and cnt[T - 1, 1] >= 1    # tiles 8.. start at chunk 1
    assert_no_wave_overflows(cnt)
    solve_and_check([(src, dst)], BETA / 2)


def test_three_chunks_second_round_counted_segment_and_an_empty_tile():
    assert_engineered_regimes()
    src, dst, _, _ = engineered()
    solve_and_check([(src, dst)], ENGINEERED_BETA / 2)


def test_batch_region_stride_is_shaped_by_the_largest_problem():
    """n = 130 beside n = 1100: the small problem's cells sit in an arena laid out for 18 row tiles"""
    assert_engineered_regimes()
    rng = np.random.default_rng(330)
    small = adversarial(rng, 130, 1.0, ENGINEERED_BETA)
    mins, C, adm = min_abs_d(small[0], small[1], ENGINEERED_BETA)
    cnt = items_per_cell(mins, C)
    assert adm and cnt.sum() >= 2
    assert_no_wave_overflows(cnt)
    src, dst, _, _ = engineered()
    solve_and_check([small, (src, dst)], ENGINEERED_BETA / 2)
    solve_and_check([(src, dst), small], ENGINEERED_BETA / 2)


def test_batch_of_an_admitted_and_a_not_admitted_problem():
    """FP64 route and popcount degrees beside the row-tile sweep (after
    test_gpu_k1_f16.py::test_batch_of_an_admitted_and_a_not_admitted_problem): beta = 2e-7 is far below the filter's
    resolution on a unit cloud, within it on the same cloud shrunk by 2^-13"""
    nb = 1e-7
    a = tp.synth_problem(20250603, 700, 0.5, nb)
    b = tp.synth_problem(20250604, 577, 0.5, nb * 2.0 ** 13)
    srcs, dsts = [a["src"], b["src"] * 2.0 ** -13], [a["dst"], b["dst"] * 2.0 ** -13]
    assert not admitted(srcs[0], dsts[0], nb) and admitted(srcs[1], dsts[1], nb)
    mins, C, adm = min_abs_d(cols(srcs[1]), cols(dsts[1]), 2 * nb)
    cnt = items_per_cell(mins, C)
    assert adm and any((cnt[I] >= 2).all() for I in range(8))  # the admitted problem merges two chunks' regions
    assert_no_wave_overflows(cnt)
    s = k1_only_solver(nb)
    s.solve_batch(srcs, dsts)
    for p in range(2):
        check_problem(s, p, srcs[p], dsts[p], nb)
