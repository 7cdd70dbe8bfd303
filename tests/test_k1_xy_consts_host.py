"""csrc/k1_consts.h compiled for the HOST (g++, no GPU): k1c::consts_xy and k1c::xy_shifts, the constants and the slot
shifts of the K1 filter's X / Y formulation, are the Python model's (tests/test_k1_xy_band_model.py), and the admission
test admits what it has to -- a suite that passes because every problem fell back to the FP64 body would prove nothing
about the filter."""
import functools
import importlib
import os
import subprocess
import tempfile

import numpy as np

from test_k1_f16_band_model import adversarial
from test_k1_xy_band_model import consts_xy, operands_xy, xy_shifts

tp = importlib.import_module("teaser-plusplus_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("C", "K2", "K0", "eps_y", "eps_x")


@functools.lru_cache(maxsize=None)
def program():
    out = os.path.join(tempfile.mkdtemp(prefix="k1xyconsts"), "k1_xy_consts_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "k1_xy_consts_main.cpp"), "-o", out])
    return out


def host_consts_xy(cases):
    """cases: [(beta, shift, r2 as np.float32)] -> list of dicts like the model's consts_xy(), plus "shifts" """
    args = []
    for beta, s, r2 in cases:
        args += [float(beta).hex(), str(int(s)), str(int(np.float32(r2).view(np.uint32)))]
    lines = subprocess.check_output([program()] + args, text=True).split("\n")
    res = []
    for l in lines[:len(cases)]:
        t = l.split()
        d = {k: np.float32(float.fromhex(v)) for k, v in zip(FIELDS, t)}
        d["kexp"], d["use_mfma"] = int(t[5]), int(t[6])
        d["shifts"] = tuple(int(v) for v in t[7:11])
        res.append(d)
    return res


def model_case(src, dst, beta):
    """src, dst [n, 3] -> (beta, shift, r2) of the pre-pass"""
    op = operands_xy(src, dst, beta)
    return (beta, op["s"], op["r2"])


def bench_cloud(n=2000, seed=20250523):
    pr = tp.synth_problem(seed, n, 0.95, 0.01)
    return np.ascontiguousarray(pr["src"].T), np.ascontiguousarray(pr["dst"].T)


def test_host_constants_are_the_models():
    src, dst = bench_cloud()
    cases = [model_case(src, dst, b) for b in (0.02, 0.005, 0.06, 0.1, 0.2, 2e-4, 2e-7, 0.9)]
    cases += [model_case(src * 250, dst * 250, 0.1), model_case(src * 0.02, dst * 0.02, 2e-4)]
    cases += [(0.02, 5, np.float32(np.inf)), (0.02, 5, np.float32(np.nan)), (0.02, 40, np.float32(3000.0)), (0.0, 5, np.float32(3000.0)),
              (2.0 ** -10, 0, np.float32(300.0)), (2.0 ** 8, 0, np.float32(300.0)), (0.7, 0, np.float32(8200.0))]
    got = host_consts_xy(cases)
    assert sum(h["use_mfma"] for h in got) >= 6
    for c, h in zip(cases, got):
        m = consts_xy(*c)
        assert h["use_mfma"] == m["use_mfma"] and h["kexp"] == m["kexp"], c
        assert h["shifts"] == xy_shifts(h["kexp"])
        if m["use_mfma"]:
            for k in FIELDS:  # the same f32 operations: equal up to the last-place freedom of sqrt / division libraries
                assert abs(float(h[k]) - float(m[k])) <= 2e-6 * abs(float(m[k])), (c, k)
    # the bound of eps_y is the budget's: 640 u R^2 / kappa plus the subnormal term, outward rounded (kappa = 2 at the
    # bench geometry: ra = 0, rb = 1, pb = 0)
    u = 2.0 ** -24
    r2, kappa = float(cases[0][2]), 2.0 ** got[0]["kexp"]
    assert got[0]["kexp"] == 1 and got[0]["shifts"] == (0, 1, 1, 0)
    want = 640 * u * r2 / kappa + u * (r2 ** 0.5 * (6.1 / 2 + 3.1) + 2)
    assert want <= float(got[0]["eps_y"]) <= want * 1.00001
    # the slot shifts over the whole window: the factor 2^-kexp is split exactly, and the fp16 range conditions hold
    for kexp in range(-17, 16):
        ra, rb, pa, pb = xy_shifts(kexp)
        assert ra + rb == kexp and pa + pb == kexp and ra >= -9 and rb >= -8 and pa >= -2 and -15 <= pb <= 0


def test_admits_every_geometry_the_f16_gpu_tests_expect_admitted():
    """the cases of tests/test_gpu_k1_f16.py, which asserts their admission by k1c::consts: the filter must run on
    them under consts_xy as well, and refuse the one they expect refused"""
    T = lambda pr, f=1.0: (np.ascontiguousarray(pr["src"].T) * f, np.ascontiguousarray(pr["dst"].T) * f)
    cases = [model_case(*T(tp.synth_problem(20250601 + n, n, 0.8, 0.01)), 0.02) for n in (64, 65, 257, 513, 2049)]
    cases += [model_case(*T(tp.synth_problem(20250602, 512, 0.8, 0.01), 2.0 ** k), 0.02 * 2.0 ** k) for k in (-20, -8, 8, 20)]
    cases.append(model_case(*adversarial(np.random.default_rng(31), 512, 1.0, 0.02, axes=(1.0, 1.0, 1e-4)), 0.02))
    for scale, nb in ((1.0, 0.01), (250.0, 0.05), (0.02, 1e-4)):
        cases.append(model_case(*adversarial(np.random.default_rng(32), 1024, scale, 2 * nb), 2 * nb))
    cases.append(model_case(*T(tp.synth_problem(20250604, 900, 0.5, 1e-7 * 2.0 ** 13), 2.0 ** -13), 2e-7))
    src, dst = T(tp.synth_problem(20250523 + 16, 1500, 0.8, 0.01))
    cases.append(model_case(src + np.array([1e4, -2e4, 3e4]), dst + np.array([-5e3, 7e3, 1e3]), 0.02))
    assert all(g["use_mfma"] == 1 for g in host_consts_xy(cases))
    assert host_consts_xy([model_case(*T(tp.synth_problem(20250603, 700, 0.5, 1e-7)), 2e-7)])[0]["use_mfma"] == 0


def test_admission_holds_where_the_filter_must_run():
    src, dst = bench_cloud()
    # the bench geometry (beta = 2 x noise bound 0.01) and its exact power-of-two rescalings
    cases = [model_case(src * 2.0 ** k, dst * 2.0 ** k, 0.02 * 2.0 ** k) for k in range(-20, 21)]
    got = host_consts_xy(cases)
    assert all(g["use_mfma"] == 1 for g in got)
    assert len({(float(g["C"]), g["kexp"]) for g in got}) == 1  # the normalised system does not see the rescaling
    # the three scales of the adversarial-band tests
    rng = np.random.default_rng(17)
    adv = []
    for scale, nb in ((1.0, 0.01), (250.0, 0.05), (0.02, 1e-4)):
        s, d = adversarial(rng, 2048, scale, 2 * nb)
        adv.append(model_case(s, d, 2 * nb))
    assert all(g["use_mfma"] == 1 for g in host_consts_xy(adv))
    # beta = 2e-7 on a unit cloud: far below the filter's resolution
    u = np.random.default_rng(3).uniform(size=(1000, 3))
    assert host_consts_xy([model_case(u, u[::-1].copy(), 2e-7)])[0]["use_mfma"] == 0
