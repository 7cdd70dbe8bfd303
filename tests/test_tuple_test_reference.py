"""The numpy restatement of the tuple-test contract (tuple_test_reference.py) equals the host function
teaser_hip_tuple_test on the problems the GPU tests use.  No GPU is needed: this pins the specification the batched
call (test_gpu_tuple_test.py) is held to, and the survivor counts written into that file."""
import importlib

import numpy as np
import pytest

import tuple_test_reference as R

tp = importlib.import_module("teaser-plusplus_amd")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("seed, survivors", [(11, 248), (12, 261), (13, 250)])
def test_scene_equals_the_host_function(seed, survivors):
    src, dst, pairs = R.scene()
    assert len(pairs) == 320
    host = R.as_array(tp.tuple_test(src, dst, pairs, R.SCALE, seed))
    assert len(host) == survivors
    assert same(R.tuple_test(src, dst, pairs, R.SCALE, seed), host)


def test_prefixes_and_suffixes_equal_the_host_function():
    src, dst, pairs = R.scene()
    got = []
    for part in [pairs[:n] for n in (1, 2, 3, 4, 5, 8, 63, 64, 65, 257)] + [pairs[-n:] for n in (63, 64, 65, 257)]:
        host = R.as_array(tp.tuple_test(src, dst, part, R.SCALE, 11))
        assert same(R.tuple_test(src, dst, part, R.SCALE, 11), host)
        got.append(len(host))
    # one or two correspondences: every triple repeats an index, a side has length 0 and the strict < fails
    assert got == [0, 0, 3, 4, 5, 8, 63, 64, 65, 234, 5, 6, 3, 188]


def test_unsorted_repeated_coincident_and_skipped_problems():
    src, dst, pairs = R.scene()
    rev = R.reversed_with_repeats()
    host = R.as_array(tp.tuple_test(src, dst, rev, R.SCALE, 11))
    assert len(rev) == 330 and len(host) == 264 and same(R.tuple_test(src, dst, rev, R.SCALE, 11), host)
    csrc, cdst, _ = R.coincident_scene()
    assert same(R.tuple_test(csrc, cdst, pairs, R.SCALE, 11), R.as_array(tp.tuple_test(csrc, cdst, pairs, R.SCALE, 11)))
    for scale in (0.0, -1.0, float("nan")):  # !(tuple_scale > 0): untouched, neither sorted nor made unique
        assert same(R.tuple_test(src, dst, rev, scale, 11), rev)
        assert same(R.as_array(tp.tuple_test(src, dst, rev, scale, 11)), rev)
    assert R.tuple_test(src, dst, [], R.SCALE, 11).shape == (0, 2)
    with pytest.raises(ValueError, match="outside"):
        R.tuple_test(src, dst, [(0, 400)], R.SCALE, 11)


def test_large_problem_equals_the_host_function():
    src, dst, pairs = R.large_problem()
    host = R.as_array(tp.tuple_test(src, dst, pairs, 0.9, 3))
    assert len(pairs) == 40003 and len(host) == 37641
    assert same(R.tuple_test(src, dst, pairs, 0.9, 3), host)
    # the draws need the exact 64-bit remainder: the low 32 bits alone give other indices
    z = R.draws(3, np.arange(1, 1001, dtype=np.uint64))
    assert ((z % np.uint64(40003)) != ((z & np.uint64(0xFFFFFFFF)) % np.uint64(40003))).sum() > 900
