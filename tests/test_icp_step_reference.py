"""The 50-digit reference of one ICP step (tests/icp_step_reference.py) and its fixture
(tests/golden/icp_step_golden.npz): the fixture regenerates identically, every case's sums are exact in FP64 (asserted
with fractions.Fraction by the reference itself while it regenerates), every case with a unique answer has condition
<= 1e3, and the project's FP64 restatements (icp_reference.umeyama, icp_plane_reference.plane_step, the Generalized-ICP
restatement's gicp_step) are within their recorded error of the 50-digit step on every such case."""
import importlib.util
import os
from fractions import Fraction as Fr

import numpy as np
import pytest

import icp_plane_reference as RP
import icp_step_reference as S
from util import ROOT

_computed = {}


def computed():
    if not _computed:
        spec = importlib.util.spec_from_file_location(
            "mks", os.path.join(ROOT, "tests", "golden", "make_icp_step_golden.py"))
        mk = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mk)
        _computed.update(mk.compute())  # asserts exactness, each case's kind and cond <= 1e3 itself
    return _computed


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "icp_step_golden.npz"))


def test_fixture_regenerates_identically():
    d, g = computed(), golden()
    assert sorted(g.files) == sorted(d)
    for key in g.files:
        if key.endswith("/err_fp64"):
            continue
        assert np.array_equal(g[key], d[key], equal_nan=g[key].dtype.kind == "f"), key
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "icp_step_golden.npz")) < 1 << 20


def test_restatements_are_within_their_recorded_error_of_the_50_digit_step():
    d, g = computed(), golden()
    worst = 0.0
    for name, kind in zip(g["names"], g["kinds"]):
        rec, now = float(g[name + "/err_fp64"]), float(d[name + "/err_fp64"])
        if kind != "unique":
            assert np.isnan(rec) and np.isnan(now), name
            continue
        print("%-20s FP64 restatement vs 50 digits: %.3g (recorded %.3g), condition %.3g" % (
            name, now, rec, float(g[name + "/cond"])))
        assert now <= rec, name
        # a restatement that is right to FP64 cannot be further off than the case's condition allows
        assert rec <= 64 * 2.0 ** -52 * max(1.0, float(g[name + "/cond"])) * max(1.0, np.abs(g[name + "/T"]).max()), name
        worst = max(worst, rec)
    assert 0 < worst < 1e-12


def test_every_case_is_exact_and_every_unique_case_well_conditioned():
    g = golden()
    kinds = dict(zip(g["names"], g["kinds"]))
    assert sorted(set(kinds.values())) == ["identity", "maximiser", "unique"]
    for name, kind in kinds.items():
        method, kernel, _ = g[name + "/meta"]
        assert bool(g[name + "/exact"]) or kernel in (1, 2, 3), name  # only rational kernel weights are not dyadic
        if kind == "unique":
            assert float(g[name + "/cond"]) <= S.COND_MAX, name
            assert np.isfinite(g[name + "/T"]).all()
        elif kind == "identity":
            assert method != S.POINT and np.isinf(g[name + "/cond"])
        else:
            assert method == S.POINT and int(g[name + "/rank"]) <= 1
    # the branches the cases are there for
    assert int(g["pt_mirror_slab/d"]) == -1 and g["pt_mirror_slab/sv"][1] > g["pt_mirror_slab/sv"][2] > 0
    assert np.array_equal(g["pt_isotropic/sv"], [2.0, 2.0, 2.0])
    assert int(g["pt_all_to_one/rank"]) == 0 and int(g["pt_5_collinear/rank"]) == 1 and int(g["pt_2/rank"]) == 1
    assert int(g["pt_3_triangle/rank"]) == 2 and int(g["pt_4_coplanar/rank"]) == 2
    assert int(g["gi_mixed_singular/skipped"]) == 21 and int(g["gi_all_singular/skipped"]) == 64
    assert np.array_equal(g["pl_zero_residuals/T"], np.eye(4))
    assert int(g["gpt_768_gap/cnt"]) == 512 and (g["gpt_768_gap/match"][256:512] == -1).all()
    assert int(g["gpl_512_last/cnt"]) == 1 and g["gpl_512_last/match"][511] == 0
    assert int(g["gpt_65793/cnt"]) == S.BIG_N == 257 * 256 + 1 and int(g["gpl_65793/cnt"]) == S.BIG_N


def test_kernel_edges_sit_exactly_on_the_threshold():
    for c in S.plane_cases():
        if c["name"] not in ("pl_huber_edge", "pl_tukey_edge"):
            continue
        s = S.exact_sums(c)
        k = Fr(c["k"])
        res = set(s["residuals"])
        for v in (k, -k, k + Fr(1, 64), -k - Fr(1, 64), k - Fr(1, 64), -k + Fr(1, 64), 2 * k):
            assert v in res, (c["name"], v)
        assert S.weight_exact(c["kernel"], c["k"], k) == (1 if c["kernel"] == 1 else 0)
        assert S.weight_exact(c["kernel"], c["k"], k + Fr(1, 64)) == (k / (k + Fr(1, 64)) if c["kernel"] == 1 else 0)
        for v in res:  # the FP64 restatement's weights are these, rounded
            assert abs(float(RP.weight(RP.KERNELS[c["kernel"]], c["k"], float(v))) -
                       float(S.weight_exact(c["kernel"], c["k"], v))) <= 2.0 ** -52


def test_integer_and_fraction_arithmetic_give_the_same_sums():
    cases = {c["name"]: c for c in S.small_cases()}
    for name in ("pt_mirror_slab", "pl_patch", "gpl_257", "gpt_768_gap"):
        a, b = S.exact_sums(cases[name], "int"), S.exact_sums(cases[name], "fraction")
        for key in ("cnt", "d2", "centre", "sp", "sq", "spq", "A", "g"):
            assert a.get(key) == b.get(key), (name, key)


def test_reference_steps_against_closed_forms():
    ctx = S.context()
    # a signed permutation of a generic cloud is recovered to the working precision
    X = S.lattice(3, 3, 3, (-1, -1, -1)) + np.array([0.5, 0.25, 0.125])
    T = S.signed_permutation((16, -32, 8))
    c = S._case("perm", S.POINT, X, X @ T[:3, :3].T + T[:3, 3], r=8.0)
    c["Q"] = c["Q"][:1]  # (the matcher needs forced pairs: use the sums directly instead)
    Xo, Qo = S._obj(X, None), S._obj(X @ T[:3, :3].T + T[:3, 3], None)
    s = dict(cnt=27, centre=[Fr(0)] * 3, sp=list(Xo.sum(0)), sq=list(Qo.sum(0)),
             spq=[[(Xo[:, r] * Qo[:, q]).sum() for q in range(3)] for r in range(3)])
    st = S.umeyama_step(ctx, s)
    assert st["unique"] and st["rank"] == 3 and st["d"] == 1
    assert max(abs(st["U"][r, q] - T[r, q]) for r in range(3) for q in range(4)) < ctx.mpf(10) ** -45
    # the exact LDL^T against a dense solve, and its pivot rule
    rng = np.random.default_rng(3)
    M = rng.integers(-8, 9, size=(12, 6))
    A = [[Fr(int(v)) for v in row] for row in M.T @ M]
    g = [Fr(int(v), 4) for v in rng.integers(-8, 9, size=6)]
    xi = S.ldl_solve(A, g)
    assert np.allclose([float(v) for v in xi], np.linalg.solve(M.T @ M, -np.array([float(v) for v in g])), rtol=1e-10)
    assert all(sum(A[r][q] * xi[q] for q in range(6)) == -g[r] for r in range(6))  # exact
    A[2] = [Fr(0)] * 6
    for r in range(6):
        A[r][2] = Fr(0)
    assert S.ldl_solve(A, g) is None


def test_contract_text_names_what_the_step_tests_pin_down():
    header = open(os.path.join(ROOT, "include", "teaser_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (header, design):
        flat = " ".join(text.replace("*", " ").split())
        assert "rank <= 1" in flat and "a maximiser" in flat
        assert "zero only up to rounding" in flat
        assert "exactly singular system gives the identity" in flat
