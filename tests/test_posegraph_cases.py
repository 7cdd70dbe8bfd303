"""The scenarios of tests/posegraph_cases.py on the CPU: each one used on the GPU meets the margin conditions in the
numpy restatement (gain ratios away from 0, stop tests that do not fire a factor 2 from their thresholds, uncertain
edges' weights a factor 2 from the pruning threshold, float64 and longdouble taking the same decisions), and each class
is what its name says.  No GPU."""
import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_reference as G

SMALL = [name for name in PC.CASES if name != "size_128"]


def test_longdouble_is_wider_than_double():
    assert PC.WIDE


@pytest.mark.parametrize("name", list(PC.CASES))
def test_scenario_meets_the_margin_conditions(name):
    start, edges, opt = PC.build(name)
    o64, old = PC.reference(name)
    assert PC.margin_problems(name, o64, old, opt) == []
    err = float(np.abs(o64["poses"].astype(np.longdouble) - old["poses"]).max()) if len(start) else 0.0
    print("%s: n %d m %d status %d iterations %s trials %s pruned %s float64 against longdouble %.3g" % (
        name, len(start), len(edges), o64["status"], o64["iterations"], [len(r) for r in PC.trials_of(o64)],
        np.flatnonzero(o64["pruned"]).tolist(), err))


def test_classes_are_what_they_claim():
    ref = {name: PC.reference(name)[0] for name in SMALL}
    assert len(PC.build("n2_m1")[0]) == 2 and len(PC.build("n2_m1")[1]) == 1
    assert not ref["consistent"]["pruned"].any() and ref["gross_chord"]["pruned"].tolist() == [k == 8 for k in range(10)]
    for name in ("reference_3", "reference_last"):
        start, _, opt = PC.build(name)
        assert np.array_equal(ref[name]["poses"][opt["reference_node"]], start[opt["reference_node"]])
    assert PC.build("reference_last")[2]["reference_node"] == len(PC.build("reference_last")[0]) - 1
    # class 4: at least three rejected trials, an acceptance after a rejection, and convergence
    flags = [t["accepted"] for rows in PC.trials_of(ref["far_start"]) for t in rows]
    assert flags.count(False) >= 3 and any(a and not b for a, b in zip(flags[1:], flags[:-1]))
    far = ref["far_start"]
    assert far["status"] in (G.RIGHT_TERM, G.INCREMENT) or (far["status"] == G.RESIDUAL and far["F"] < 1e-6)
    assert not np.array_equal(PC.build("realistic")[1][0][3], np.eye(6))
    # class 6: N on both sides of the tile's first two edges, an exact multiple, n = 128
    T = PC.tile_constant()
    N = sorted(6 * (int(name[5:]) - 1) for name in PC.SIZE_CASES)
    for edge in (T, 2 * T):
        assert max(v for v in N if v < edge) > edge - 6 and min(v for v in N if v > edge) < edge + 6
    assert any(v % T == 0 for v in N) and N[-1] == 6 * 127
    # class 7: a doubled pair, its reverse, and a node without an edge that does not move
    start, edges, _ = PC.build("multi_edge")
    pairs = [(E[0], E[1]) for E in edges]
    assert pairs.count((2, 1)) == 2 and pairs.count((1, 2)) == 1 and all(5 not in p for p in pairs)
    assert np.array_equal(ref["multi_edge"]["poses"][5], start[5])
    # class 8: every factorisation fails and the poses come back bit-equal
    neg = ref["negative_information"]
    assert neg["status"] == G.MAX_ITERATION_LM and neg["iterations"] == [0, 0]
    assert all(t["rho"] is None for rows in PC.trials_of(neg) for t in rows) and len(PC.trials_of(neg)[0]) == 20
    assert np.array_equal(neg["poses"], PC.build("negative_information")[0])
    assert ref["max_iteration_1"]["status"] == G.MAX_ITERATION
    one = ref["no_pruning"]
    assert len(one["passes"]) == 1 and not one["pruned"].any() and one["confidence"][8] < 0.25
    for name in PC.TRIVIAL:
        assert ref[name]["status"] == G.TRIVIAL
