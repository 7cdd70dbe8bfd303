"""The numpy restatement of the RANSAC contract (tests/ransac_reference.py) alone, without a GPU: its draws are the
tuple test's, it recovers the planted exact pose, it implements the stop rule's special cases as IEEE lets them fall,
it does not depend on how its trials are asked for, and the committed fixture produces the behaviours the GPU tests
rely on (tests/golden/make_ransac_golden.py asserted them when it wrote the fixture)."""
import math
import os

import numpy as np
import pytest

import ransac_reference as RR
import tuple_test_reference as TT
from util import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "ransac_golden.npz"))
COND_MAX = 1e3


def case(name):
    r, s, d = G[name + "/params"]
    return dict(P=G[name + "/P"], Q=G[name + "/Q"], corr=G[name + "/corr"], r=float(r), s=float(s), d=float(d),
                seed=int(G[name + "/seed"][0]), ransac_n=int(G[name + "/ransac_n"]))


def test_draws_are_the_tuple_tests():
    seed = 0x5EED
    want = TT.draws(seed, np.arange(1, 31, dtype=np.uint64))
    got = np.array([RR.draw(seed, m + 1) for m in range(30)], dtype=np.uint64)
    assert np.array_equal(want, got)
    smp = RR.samples(seed, 3, 7, 2, 4)
    assert smp.tolist() == [[RR.draw(seed, 3 * i + k + 1) % 7 for k in range(3)] for i in range(2, 6)]


def test_fixture_shapes_and_caps():
    assert [len(G[n + "/corr"]) for n in G["trial_cases"]] == [3, 48, 255, 256, 257] and len(G["tiny2/corr"]) == 2
    for name in G["trial_cases"]:
        for key in ("P", "Q"):
            assert np.array_equal(G[name + "/" + key] * 1024, np.round(G[name + "/" + key] * 1024))  # the dyadic grid
        cond = G[name + "/cond"]
        assert cond.shape == (int(G["trials"]),) == (2048,)
        if len(G[name + "/corr"]) >= 48:
            assert (cond > COND_MAX).mean() <= 0.25
    c = case("e255")
    moved = c["P"][c["corr"][:, 0]] @ G["e255/T_true"][:3, :3].T + G["e255/T_true"][:3, 3]
    assert np.array_equal(moved[G["e255/planted"]], c["Q"][c["corr"][:, 1]][G["e255/planted"]])  # exact inliers


def test_recovers_the_planted_exact_pose():
    c = case("e255")
    out = RR.ransac(c["P"], c["Q"], c["corr"], c["r"], 3, 2048, 0.999, c["seed"])
    q = out["best_trial"]
    bar = 16.0 * max(float(G["e255/A"][q]), 2.0 ** -52 * float(G["e255/cond"][q]))
    assert out["count"] >= G["e255/planted"].sum() and 0 <= q < out["trials"] < 2048
    assert np.linalg.norm(out["transformation"] - G["e255/T_true"]) <= bar
    assert out["fitness"] == out["count"] / 255 and out["inlier_rmse"] <= 1e-12


def test_stop_rule_special_cases():
    assert RR.stop_k(1.0, 10, 100, 3) == math.inf            # confidence 1: log(0) = -inf over a negative number
    assert math.isnan(RR.stop_k(1.0, 100, 100, 3))           # ... and -inf / -inf when every pair is an inlier
    assert RR.stop_k(0.999, 100, 100, 3) == 0.0              # count = ncorr: a finite number over -inf
    assert RR.stop_k(0.999, 1, 10 ** 6, 3) == -math.inf      # 1 - 1e-18 rounds to 1: a negative number over +0
    assert RR.stop_k(0.0, 10, 100, 3) == 0.0 and math.copysign(1.0, RR.stop_k(0.0, 10, 100, 3)) < 0
    assert RR.stop_k(0.999, 50, 100, 3) == math.log(1 - 0.999) / math.log(1 - math.pow(0.5, 3.0))

    def records(counts):
        n = len(counts)
        return lambda first, m: dict(flags=np.full(m, 7, np.uint8), count=np.array(counts[first:first + m]),
                                     sum_d2=np.ones(m), transformation=np.tile(np.eye(4), (m, 1, 1)))

    rising = list(range(1, 41))
    out = RR.loop(records(rising), 100, 3, 40, 1.0)
    assert out["trials"] == 40 and out["best_trial"] == 39        # never stops early
    out = RR.loop(records([5, 100, 100, 100]), 100, 3, 4, 0.999)
    assert out["trials"] == 2 and out["best_trial"] == 1          # count = ncorr stops at once
    out = RR.loop(records([1] * 10), 10 ** 6, 3, 10, 0.999)
    assert out["trials"] == 1 and out["best_trial"] == 0          # k = -inf stops at once, too
    out = RR.loop(records([3, 3, 3]), 100, 3, 3, 1.0)
    assert out["best_trial"] == 0 and out["trials"] == 3          # ties stay with the earlier trial
    out = RR.loop(records([3, 3, 3]), 2, 3, 3, 1.0)
    assert out["best_trial"] == -1 and out["trials"] == 0 and np.array_equal(out["transformation"], np.eye(4))
    out = RR.loop(records([3, 3, 3]), 100, 3, 0, 1.0)
    assert out["best_trial"] == -1 and out["trials"] == 0


@pytest.mark.parametrize("name", ["early", "full"])
def test_loop_cases_behave_as_the_fixture_says_whatever_the_chunk(name):
    c = case(name)
    max_iteration, confidence = int(G[name + "/criteria"][0]), float(G[name + "/criteria"][1])
    outs = [RR.ransac(c["P"], c["Q"], c["corr"], c["r"], c["ransac_n"], max_iteration, confidence, c["seed"], c["s"],
                      c["d"], chunk=chunk) for chunk in (64, 256, 4096)]
    for o in outs[1:]:
        assert all(np.array_equal(o[k], outs[0][k]) for k in outs[0])
    out = outs[0]
    assert 0 < out["valid_trials"] < out["trials"] and out["best_trial"] >= 0
    if name == "early":
        assert 64 < out["trials"] < max_iteration and out["trials"] % 64 != 0
    else:
        assert out["trials"] == max_iteration


def test_score_sums_in_blocks_of_256():
    """The stated order is not the plain left-to-right sum: a record set where the two differ tells them apart."""
    rng = np.random.default_rng(5)
    rec = np.concatenate([rng.normal(size=(300, 3)), np.zeros((300, 3))], 1)
    rec[:, 3:] = rec[:, :3] + rng.normal(scale=1e-3, size=(300, 3))
    count, total, inl = RR.score(np.eye(4)[None], rec, 1.0)
    d2 = RR.d2_of(np.eye(4)[None], rec)[0]
    want = (0.0 + np.cumsum(d2[:256])[-1]) + np.cumsum(d2[256:])[-1]
    assert count[0] == 300 and inl.all() and total[0] == want
