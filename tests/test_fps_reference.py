"""The numpy restatement of farthest-point down-sampling (tests/fps_reference.py) against itself: the per-round
vectorised form equals the literal scalar loop on lattices (ties and repeats) and on float clouds, sel_dist and
final_dist mean what the contract says, sel_dist never grows after the first sample, and a cloud with fewer distinct
positions than samples repeats its last one."""
import numpy as np
import pytest

import fps_reference as RF


def same(a, b):
    return all(np.array_equal(x, y) and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 65, 130, 300])
def test_vectorised_form_equals_the_scalar_loop_on_lattices(n):
    rng = np.random.default_rng(n)
    P = RF.lattice(rng, n, side=3 if n < 64 else 6)
    for K in sorted({0, 1, min(n, 5), n}):
        for s in sorted({0, n // 2, n - 1}):
            assert same(RF.fps(P, K, s), RF.fps_literal(P, K, s)), (n, K, s)


@pytest.mark.parametrize("n,K", [(50, 50), (257, 40)])
def test_vectorised_form_equals_the_scalar_loop_on_float_clouds(n, K):
    P = RF.gaussian(np.random.default_rng(7 * n), n)
    assert same(RF.fps(P, K, 3), RF.fps_literal(P, K, 3))


@pytest.mark.parametrize("scene", ["lattice", "gaussian", "three"])
def test_distance_outputs_mean_what_the_contract_says(scene):
    rng = np.random.default_rng(11)
    P = {"lattice": RF.lattice(rng, 400), "gaussian": RF.gaussian(rng, 400), "three": RF.three_positions(60)}[scene]
    K = 25
    index, sel, fin = RF.fps(P, K, 5)
    assert index[0] == 5 and sel[0] == np.inf
    assert sel.tobytes() == RF.brute_sel_dist(P, index).tobytes()
    assert fin.tobytes() == RF.brute_final_dist(P, index).tobytes()
    assert (np.diff(sel[1:]) <= 0).all()  # a later sample is never farther from the set than an earlier one was
    assert (fin <= sel[-1]).all() and (fin[index] == 0).all()


def test_fewer_distinct_positions_than_samples_repeat_the_last_sample():
    index, sel, fin = RF.fps(RF.identical(), 5, 7)
    assert index.tolist() == [7, 7, 7, 7, 7]
    assert sel.tolist() == [np.inf, 0, 0, 0, 0] and (fin == 0).all()
    P = RF.three_positions()
    index, sel, fin = RF.fps(P, 6, 4)
    assert len(set(index[:3].tolist())) == 3 and index[3:].tolist() == [index[2]] * 3
    assert {tuple(p) for p in P[index[:3]]} == {tuple(p) for p in P[:3]}
    assert (sel[1:3] > 0).all() and (sel[3:] == 0).all() and (fin == 0).all()
    assert same(RF.fps(P, 6, 4), RF.fps_literal(P, 6, 4))


def test_ties_go_to_the_smallest_index_and_infinite_distances_are_ordinary():
    P = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]])
    assert RF.fps(P, 3, 0)[0].tolist() == [0, 1, 2]  # 1, 2, 3 and 4 tie at d2 = 1; then 2 and 3 tie at d2 = 1
    Q = np.array([[0.0, 0, 0], [1e200, 0, 0], [-1e200, 0, 0], [0, 1e200, 0]])
    index, sel, fin = RF.fps(Q, 3, 0)
    assert index.tolist() == [0, 1, 2] and sel[1] == np.inf and sel[2] == np.inf
    assert same(RF.fps(Q, 4, 0), RF.fps_literal(Q, 4, 0))


def test_a_large_case_is_quick():
    P = RF.lattice(np.random.default_rng(3), 12289)
    index, sel, fin = RF.fps(P, 64, 12288)
    assert index[0] == 12288 and len(set(index.tolist())) == 64


def test_the_grid_of_the_cxx_example():
    """tests/cxx/fps_example.cpp carries these numbers as literals."""
    P = np.array([[i % 5, i // 5, 0] for i in range(25)], dtype=np.float64)
    index, sel, fin = RF.fps(P, 5, 12)
    assert index.tolist() == [12, 0, 4, 20, 24] and sel.tolist() == [np.inf, 8, 8, 8, 8]
    assert fin.max() == 4 and fin[12] == 0 and fin[2] == 4
    index, _, _ = RF.fps(P, 25, 3)
    assert index[0] == 3 and sorted(index.tolist()) == list(range(25))
