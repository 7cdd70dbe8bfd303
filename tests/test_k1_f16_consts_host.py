"""csrc/k1_consts.h compiled for the HOST (g++, no GPU): the constants the device code computes are the Python model's
(tests/test_k1_f16_band_model.py), and the admission test admits what it has to -- a suite that passes because every
problem fell back to the FP64 body would prove nothing about the filter."""
import importlib

import numpy as np

from k1_f16_host import FIELDS, host_consts, host_shift
from test_k1_f16_band_model import adversarial, consts, half_extent, operands

tp = importlib.import_module("teaser-plusplus_amd")


def model_case(src, dst, beta):
    """src, dst [n, 3] -> (beta, shift, r2) of the pre-pass"""
    op = operands(src, dst, beta)
    return (beta, op["s"], op["r2"])


def bench_cloud(n=2000, seed=20250523):
    pr = tp.synth_problem(seed, n, 0.95, 0.01)
    return np.ascontiguousarray(pr["src"].T), np.ascontiguousarray(pr["dst"].T)


def test_host_constants_are_the_models():
    rng = np.random.default_rng(41)
    src, dst = bench_cloud()
    cases = [model_case(src, dst, b) for b in (0.02, 0.005, 0.06, 0.2, 2e-7, 0.9)]
    cases += [model_case(src * 250, dst * 250, 0.1), model_case(src * 0.02, dst * 0.02, 2e-4)]
    cases += [(0.02, 5, np.float32(np.inf)), (0.02, 5, np.float32(np.nan)), (0.02, 40, np.float32(3000.0)), (0.0, 5, np.float32(3000.0))]
    got = host_consts(cases)
    for c, h in zip(cases, got):
        m = consts(*c)
        assert h["use_mfma"] == m["use_mfma"] and h["kexp"] == m["kexp"], c
        if m["use_mfma"]:
            for k in FIELDS:  # the same f32 operations: equal up to the last-place freedom of sqrt / division libraries
                assert abs(float(h[k]) - float(m[k])) <= 2e-6 * abs(float(m[k])), (c, k)
    # the model's bound of eps_u is the budget's: 500 u R^2 plus the subnormal term, outward rounded
    u = 2.0 ** -24
    r2 = float(cases[0][2])
    assert 500 * u * r2 + u * (12.1 * r2 ** 0.5 + 1) <= float(got[0]["eps_u"]) <= (500 * u * r2 + u * (12.1 * r2 ** 0.5 + 1)) * 1.00001
    for H in (1.0, 0.999, 31.9, 32.0, 1e-6, 3e7):
        s = host_shift(H)
        assert 16.0 <= H * 2.0 ** s < 32.0


def test_admission_holds_where_the_filter_must_run():
    src, dst = bench_cloud()
    # the bench geometry (beta = 2 x noise bound 0.01) and its exact power-of-two rescalings
    cases = [model_case(src * 2.0 ** k, dst * 2.0 ** k, 0.02 * 2.0 ** k) for k in range(-20, 21)]
    got = host_consts(cases)
    assert all(g["use_mfma"] == 1 for g in got)
    assert len({(float(g["C"]), g["kexp"]) for g in got}) == 1  # the normalised system does not see the rescaling
    # the three scales of test_k1_filter_adversarial_band
    rng = np.random.default_rng(17)
    adv = []
    for scale, nb in ((1.0, 0.01), (250.0, 0.05), (0.02, 1e-4)):
        s, d = adversarial(rng, 2048, scale, 2 * nb)
        adv.append(model_case(s, d, 2 * nb))
    assert all(g["use_mfma"] == 1 for g in host_consts(adv))
    # beta = 2e-7 on a unit cloud: far below the filter's resolution
    u = np.random.default_rng(3).uniform(size=(1000, 3))
    assert host_consts([model_case(u, u[::-1].copy(), 2e-7)])[0]["use_mfma"] == 0
