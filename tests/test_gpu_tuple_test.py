"""GPU tests of the batched tuple test (teaser_hip_features_tuple_test_batch; csrc/features.hip, kernels_features.hip:
feat_tuple_batch_kernel).  The contract (include/teaser_hip.h, "tuple_test_batch") is identity with the host function
teaser_hip_tuple_test for the same problem and non-zero seed, so every comparison is exact equality with
tp.tuple_test: no tolerance appears.  The problems are those of tuple_test_reference.py, which
test_tuple_test_reference.py pins to the same host function without a GPU.

Survivor counts of the host function on them: the scene 248 / 261 / 250 for seeds 11 / 12 / 13 (they differ, so a seed
mix-up shows); its prefixes of 1, 2, 3, 4, 5, 8, 63, 64, 65, 257 pairs 0, 0, 3, 4, 5, 8, 63, 64, 65, 234; its last 63,
64, 65, 257 pairs 5, 6, 3, 188 (mostly wrong pairs: sparse flags); reversed with repeats 264; 40 003 pairs 37 641."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import tuple_test_reference as R
from util import ROOT

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")
feat = importlib.import_module("teaser-plusplus_amd.features")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def host(src, dst, pairs, scale, seed):
    return R.as_array(tp.tuple_test(src, dst, pairs, scale, seed))


@pytest.mark.parametrize("seed, survivors", [(11, 248), (12, 261), (13, 250)])
def test_scene_equals_the_host_function(seed, survivors):
    src, dst, pairs = R.scene()
    got = tp.tuple_test_batch([src], [dst], [pairs], R.SCALE, seed)
    assert len(got) == 1 and len(got[0]) == survivors
    assert same(got[0], host(src, dst, pairs, R.SCALE, seed))


def test_prefixes_and_suffixes_in_one_batch():
    """ncorr = 1 and 2 (no triple can pass), 3 .. 8 (every draw collides), 63 / 64 / 65 (one wavefront of pairs) and
    257 (beyond one block's worth of flags), from the consistent head of the list and from its mostly wrong tail."""
    src, dst, pairs = R.scene()
    parts = [pairs[:n] for n in (1, 2, 3, 4, 5, 8, 63, 64, 65, 257)] + [pairs[-n:] for n in (63, 64, 65, 257)]
    got = tp.tuple_test_batch([src] * len(parts), [dst] * len(parts), parts, R.SCALE, 11)
    for part, g in zip(parts, got):
        assert same(g, host(src, dst, part, R.SCALE, 11)), len(part)
    assert [len(g) for g in got] == [0, 0, 3, 4, 5, 8, 63, 64, 65, 234, 5, 6, 3, 188]


def test_mixed_batch_equals_single_problem_calls():
    """Two seeds, an empty problem, a skipped one (scale 0: its unsorted input comes back untouched), an unsorted list
    with repeats and a scene with coincident points in one call; each problem alone gives the same bytes, and so does
    the call cut into one wave per problem."""
    src, dst, pairs = R.scene()
    rev = R.reversed_with_repeats()
    csrc, cdst, _ = R.coincident_scene()
    none = np.zeros((0, 2), dtype=np.int32)
    srcs = [src, src, src, src, src, csrc]
    dsts = [dst, dst, dst, dst, dst, cdst]
    prs = [pairs, pairs, none, rev, rev, pairs]
    scales = [R.SCALE, R.SCALE, R.SCALE, 0.0, R.SCALE, R.SCALE]
    seeds = [11, 12, 11, 11, 11, 11]
    got = tp.tuple_test_batch(srcs, dsts, prs, scales, seeds)
    assert len(got) == 6
    for k in (0, 1, 4, 5):
        assert same(got[k], host(srcs[k], dsts[k], prs[k], scales[k], seeds[k])), k
    assert [len(g) for g in got] == [248, 261, 0, 330, 264, 248]
    assert got[2].shape == (0, 2) and same(got[3], rev)
    for k in range(6):
        alone = tp.tuple_test_batch([srcs[k]], [dsts[k]], [prs[k]], scales[k], seeds[k])
        assert same(alone[0], got[k]), k
    h = feat._handle()
    h._set_budget(None, 8 * 320)  # room for 320 pairs: a wave per problem
    try:
        split = tp.tuple_test_batch(srcs, dsts, prs, scales, seeds)
    finally:
        h._set_budget(None, None)
    assert all(same(a, b) for a, b in zip(split, got))


def test_large_problem_grid_stride_and_64_bit_remainder():
    """4 000 300 trials: more than the problem's blocks hold at one trial per lane, and draws that need the exact
    64-bit remainder (test_tuple_test_reference.py).  A small problem beside it shares the grid."""
    cloud, _, pairs = R.large_problem()
    src, dst, small = R.scene()
    got = tp.tuple_test_batch([cloud, src], [cloud, dst], [pairs, small], [0.9, R.SCALE], [3, 13])
    want = host(cloud, cloud, pairs, 0.9, 3)
    assert len(want) == 37641 and same(got[0], want)
    assert same(got[1], host(src, dst, small, R.SCALE, 13))


def test_seed_zero_draws_from_the_clock():
    src, dst, pairs = R.scene()
    got = tp.tuple_test_batch([src], [dst], [pairs], R.SCALE)[0]
    rows = [tuple(r) for r in got.tolist()]
    assert rows == sorted(set(rows)) and set(rows) <= set(map(tuple, pairs.tolist()))
    assert {(i, i) for i in range(200)} <= set(rows)  # every consistent pair survives, whatever the seed


def test_out_of_range_index_names_its_problem_and_writes_nothing():
    src, dst, pairs = R.scene()
    bad = pairs.copy()
    bad[100, 1] = 400
    with pytest.raises(tp.TeaserHipError, match=r"\(problem 2\)"):
        tp.tuple_test_batch([src] * 3, [dst] * 3, [pairs, pairs, bad], R.SCALE, 11)
    with pytest.raises(tp.TeaserHipError, match=r"\(problem 2\)"):
        tp.tuple_test_batch([src] * 3, [dst] * 3, [pairs, pairs, -bad], R.SCALE, 11)
    # through the C entry point: the caller's arrays are as they were
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    bufs = [pairs.copy(), pairs.copy(), bad.copy()]
    cnt = np.array([320, 320, 320], dtype=np.int64)
    n = np.array([400] * 3, dtype=np.int32)
    scale, seed = np.full(3, R.SCALE, dtype=np.float32), np.full(3, 11, dtype=np.uint64)
    h = feat._handle()
    with pytest.raises(tp.TeaserHipError, match=r"\(problem 2\)") as e:
        h.call(h._lib.teaser_hip_features_tuple_test_batch, 3, feat._ptrs([src] * 3, fp), n.ctypes.data_as(ip),
               feat._ptrs([dst] * 3, fp), n.ctypes.data_as(ip), scale.ctypes.data_as(fp),
               seed.ctypes.data_as(C.POINTER(C.c_uint64)), feat._ptrs(bufs, ip), cnt.ctypes.data_as(C.POINTER(C.c_int64)))
    assert e.value.status == 1  # TEASER_HIP_ERR_BAD_ARG
    assert cnt.tolist() == [320, 320, 320]
    assert same(bufs[0], pairs) and same(bufs[1], pairs) and same(bufs[2], bad)
    # the handle stays usable
    assert len(tp.tuple_test_batch([src], [dst], [pairs], R.SCALE, 11)[0]) == 248


def test_argument_forms():
    src, dst, pairs = R.scene()
    with pytest.raises(ValueError, match="tuple_scale"):
        tp.tuple_test_batch([src, src], [dst, dst], [pairs, pairs], [0.9, 0.9, 0.9], 11)
    with pytest.raises(ValueError, match="seed"):
        tp.tuple_test_batch([src, src], [dst, dst], [pairs, pairs], 0.9, [11])
    with pytest.raises(ValueError, match="same length"):
        tp.tuple_test_batch([src, src], [dst, dst], [pairs], 0.9, 11)
    assert tp.tuple_test_batch([], [], [], 0.9, 11) == []
    as_lists = tp.tuple_test_batch([src.tolist()], [dst.tolist()], [[tuple(r) for r in pairs.tolist()]], R.SCALE, 12)
    assert len(as_lists[0]) == 261


@pytest.fixture(scope="module")
def config5():
    C5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    a, b, vox = C5["cloud_bin_0"], C5["cloud_bin_4"], float(C5["voxel_size"])
    return [a, b], [b, a], vox


def test_correspondence_calls_with_a_tuple_scale_keep_the_host_semantics(config5):
    """correspondences_batch / correspondences_knn_batch / Matcher.calculateCorrespondencesBatch with a tuple scale =
    the same call without it, followed by the host function per pair: not a pair differs."""
    src, dst, vox = config5
    plain, feats = tp.correspondences_batch(src, dst, 2 * vox, 5 * vox, return_features=True)
    with_tuple = tp.correspondences_batch(src, dst, 2 * vox, 5 * vox, tuple_scale=0.9, tuple_seed=7)
    for b in range(2):
        want = host(src[b], dst[b], plain[b], 0.9, 7)
        assert 0 < len(want) < len(plain[b]) and same(with_tuple[b], want), b
    knn = tp.correspondences_knn_batch(src, dst, 2 * vox, 5 * vox, 4)
    knn_tuple = tp.correspondences_knn_batch(src, dst, 2 * vox, 5 * vox, 4, tuple_scale=0.9, tuple_seed=7)
    for b in range(2):
        want = host(src[b], dst[b], knn[b], 0.9, 7)
        assert len(knn[b]) > len(plain[b]) and 0 < len(want) < len(knn[b]) and same(knn_tuple[b], want), b
    one = tp.correspondences_knn(src[0], dst[0], 2 * vox, 5 * vox, 4, tuple_scale=0.9, tuple_seed=7)
    assert same(one, knn_tuple[0])
    assert same(tp.correspondences_knn(src[0], dst[0], 2 * vox, 5 * vox, 4), knn[0])  # the defaults: no tuple test
    m = tp.Matcher().calculateCorrespondencesBatch(src, dst, feats[0], feats[1], True, True, True, 0.9, 7)
    for b in range(2):
        assert m[b] == tp.tuple_test(src[b], dst[b], plain[b], 0.9, 7), b
    skipped = tp.Matcher().calculateCorrespondencesBatch(src, dst, feats[0], feats[1], True, True, False, 0.9, 7)
    assert [np.asarray(s).tolist() for s in skipped] == [p.tolist() for p in plain]
