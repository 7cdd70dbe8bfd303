"""Farthest-point down-sampling on the MI355X (teaser_hip_icp_farthest_point_down_sample_batch through the Python form)
against the numpy restatement tests/fps_reference.py: indices compared for EQUALITY, sel_dist and final_dist by their
bytes.  Every case runs on both routes -- "fps_resident_max" at its default C (read from the handle, never written
here as a number) and at 0 -- and the two must give identical bytes.  Scenes: integer lattices (exact arithmetic, ties
everywhere) at the wave, block, workgroup and capacity edges from both ends of the cloud; a planted unique farthest point
at the last lane of a wave, the first lane of the next, the last thread of the workgroup, the first slot of the next
register tile and the last slot of the last tile; N(0, 1) + 1 000 float clouds (a fused d2 would differ); clouds with
fewer distinct positions than samples; the edge sample counts; one batch of sizes 0, 1, 257, 4 097 and C + 1 that uses
both routes in one call, reversed, each alone and twice; the refusals."""
import importlib

import numpy as np
import pytest

import fps_reference as RF

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def need_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def capacity():
    """C: the default of fps_resident_max, the largest cloud the resident route serves."""
    need_gpu()
    c = tp.get_icp_option("fps_resident_max")
    assert c >= 1024, "the lattice sizes below assume a capacity of at least one point per lane"
    return c


def run(clouds, K, s):
    index, sel, fin = tp.farthest_point_down_sample_batch(clouds, K, s, return_sel_dist=True, return_final_dist=True)
    return list(zip(index, sel, fin))


def same_bytes(a, b, what):
    for x, y, part in zip(a, b, ("index", "sel_dist", "final_dist")):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: %s differ" % (what, part)


def both_routes(clouds, K, s):
    """The call at the default of fps_resident_max and with every cloud streamed: identical bytes; returns the first."""
    C = capacity()
    try:
        resident = run(clouds, K, s)
        tp.set_icp_option("fps_resident_max", 0)
        streamed = run(clouds, K, s)
    finally:
        tp.set_icp_option("fps_resident_max", C)
    for b, (r, t) in enumerate(zip(resident, streamed)):
        same_bytes(r, t, "cloud %d: resident against streamed" % b)
    return resident


def check(got, P, K, s, what):
    want = RF.fps(P, K, s)
    assert np.array_equal(got[0], want[0]), "%s: index differs" % what
    same_bytes(got, want, what)
    return want


LATTICE_N = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, "C-1", "C", "C+1"]


@pytest.mark.parametrize("size", LATTICE_N)
def test_integer_lattices_from_both_ends(size):
    C = capacity()
    n = {"C-1": C - 1, "C": C, "C+1": C + 1}.get(size, size)
    P = RF.lattice(np.random.default_rng(n), n)
    K = min(n, 48)
    got = both_routes([P, P], K, [0, n - 1])  # one call: the two starts share the launches
    for g, s in zip(got, (0, n - 1)):
        want = check(g, P, K, s, "n %d start %d" % (n, s))
        assert want[0][0] == s and want[1][0] == np.inf
    if n >= 256:
        assert len(set(got[0][0].tolist())) == K and (got[0][1][1:] > 0).all()  # 216 positions: no repeat within 48


def test_a_planted_winner_is_found_at_every_seam():
    C = capacity()
    n = C
    spots = [0, 63, 64, 1023, 1024, n - 1]
    clouds = [RF.planted(n, at, seed=at) for at in spots]
    got = both_routes(clouds, 4, 7)
    for g, P, at in zip(got, clouds, spots):
        check(g, P, 4, 7, "planted at %d" % at)
        assert g[0][0] == 7 and g[0][1] == at


@pytest.mark.parametrize("n,K", [(257, 257), (4097, 64)])
def test_float_clouds(n, K):
    need_gpu()
    P = RF.gaussian(np.random.default_rng(n), n)
    got = both_routes([P], K, 0)[0]
    check(got, P, K, 0, "gaussian n %d" % n)
    assert len(set(got[0].tolist())) == K
    if K == n:
        assert sorted(got[0].tolist()) == list(range(n)) and (got[2] == 0).all()


def test_fewer_distinct_positions_than_samples():
    need_gpu()
    same, three = RF.identical(), RF.three_positions()
    got = both_routes([same, three], [5, 6], [7, 4])
    check(got[0], same, 5, 7, "513 identical points")
    assert got[0][0].tolist() == [7, 7, 7, 7, 7]
    want = check(got[1], three, 6, 4, "600 points on 3 positions")
    assert len(set(want[0][:3].tolist())) == 3 and want[0][3:].tolist() == [want[0][2]] * 3


def test_edge_sample_counts():
    need_gpu()
    rng = np.random.default_rng(5)
    clouds = [np.zeros((0, 3)), RF.lattice(rng, 5), RF.lattice(rng, 5), RF.lattice(rng, 65), RF.gaussian(rng, 130)]
    K, s = [0, 0, 1, 65, 130], [0, 99, 4, 64, 1]  # (K = 0: start_index is not looked at)
    got = both_routes(clouds, K, s)
    for b, g in enumerate(got):
        if K[b] == 0:
            assert len(g[0]) == 0 and len(g[1]) == 0 and (g[2] == 0).all()  # nothing written: the wrapper's zeros
        else:
            check(g, clouds[b], K[b], s[b], "cloud %d" % b)
    assert got[2][0].tolist() == [4]
    assert sorted(got[4][0].tolist()) == list(range(130))
    assert tp.farthest_point_indices(clouds[0], 0).shape == (0,)
    # the Python form: K == n returns the cloud itself in input order (Open3D's shortcut), else the samples in order
    assert np.array_equal(tp.farthest_point_down_sample(clouds[4], 130, 1), clouds[4])
    assert np.array_equal(tp.farthest_point_down_sample(clouds[4], 9, 1), clouds[4][RF.fps(clouds[4], 9, 1)[0]])
    assert np.array_equal(tp.farthest_point_indices(clouds[4], 9, 1), RF.fps(clouds[4], 9, 1)[0])


def test_batch_positions_and_repetition_give_identical_bits():
    C = capacity()
    rng = np.random.default_rng(99)
    clouds = [np.zeros((0, 3)), RF.lattice(rng, 1), RF.lattice(rng, 257), RF.gaussian(rng, 4097), RF.lattice(rng, C + 1)]
    K, s = [0, 1, 33, 64, 17], [0, 0, 256, 2000, C]
    fwd = run(clouds, K, s)  # the default option: the first four resident, the last streamed
    rev = run(clouds[::-1], K[::-1], s[::-1])[::-1]
    again = run(clouds, K, s)
    for b in range(1, 5):
        check(fwd[b], clouds[b], K[b], s[b], "cloud %d in the batch" % b)
        alone = run([clouds[b]], K[b], s[b])[0]
        for other, what in ((rev[b], "reversed batch"), (again[b], "second call"), (alone, "alone")):
            same_bytes(fwd[b], other, "cloud %d: %s" % (b, what))
    assert len(fwd[0][0]) == 0
    # the optional outputs one at a time
    index = tp.farthest_point_down_sample_batch(clouds, K, s)
    index2, sel = tp.farthest_point_down_sample_batch(clouds, K, s, return_sel_dist=True)
    index3, fin = tp.farthest_point_down_sample_batch(clouds, K, s, return_final_dist=True)
    for b in range(5):
        assert index[b].tobytes() == index2[b].tobytes() == index3[b].tobytes() == fwd[b][0].tobytes()
        assert sel[b].tobytes() == fwd[b][1].tobytes()
        if K[b]:
            assert fin[b].tobytes() == fwd[b][2].tobytes()


def test_refusals_name_the_argument():
    C = capacity()
    P = RF.lattice(np.random.default_rng(1), 40)
    bad = P.copy()
    bad[3, 1] = np.nan
    for args, word in (((P, 41), "num_samples"), ((P, -1), "num_samples"), ((P, 5, 40), "start_index"),
                       ((P, 5, -1), "start_index"), ((bad, 5), "points")):
        with pytest.raises(tp.TeaserHipError, match=word):
            tp.farthest_point_indices(*args)
    with pytest.raises(tp.TeaserHipError, match="fps_resident_max"):
        tp.set_icp_option("fps_resident_max", C + 1)
    assert tp.get_icp_option("fps_resident_max") == C
    check(run([P], 5, 39)[0], P, 5, 39, "after the refusals")
