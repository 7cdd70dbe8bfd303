"""CPU model of the K1 filter in its X / Y formulation (csrc/kernels_graph.hip, csrc/k1_consts.h "The X / Y
formulation"): two chained MFMAs per quarter tile leave X = -A / kappa (first link) and Y = u / kappa
(second link), and the kernel's d is Y^2 + X = (u^2 + w) / kappa^2.

A numpy restatement of the new slot table (every value shifted by an exact power of two before it is split into fp16
pieces), of k1c::consts_xy and of an f32 accumulation of the chain under the documented hardware model (exact
products, every addition rounded to f32, several orders), in the style of test_k1_f16_band_model.py, whose helpers it
imports.  It pins the slot table and the constants: every operand is an exact fp16 and every product an exact f32, a
pair the constant band trusts gets the reference's answer, short pairs and self pairs are never trusted, a
power-of-two rescaling packs the same bits, subnormal low pieces are covered, and the admission test admits what it
has to and refuses what the fp16 range or the budget cannot hold.  (The GPU tests check the real instruction.)"""
import math

import numpy as np

import test_k1_f16_band_model as old
from test_k1_band_model import reference_edge
from test_k1_f16_band_model import (F16_MAX, K_EPS_A, K_SHORT_RATIO, U, accumulate, adversarial, bench_like, f16, f32,
                                    half_extent, norm_shift, scale2, split3)

K_EPS_Y = f32(640.0)


def xy_shifts(kexp):
    """k1c::xy_shifts: coordinates 2^-ra (row) x 2^-rb (column), norms 2^-pa against 2^-pb"""
    ra = kexp >> 1
    pa = max(kexp, -2)
    return ra, kexp - ra, pa, kexp - pa


def pack_xy(sp, dp, kexp):
    """normalised centred f32 points -> row side A [n, 32], column side B [n, 32] (f32 arrays of the fp16 values)"""
    ra, rb, pa, pb = xy_shifts(kexp)
    fra, frb, fpa, P = f32(2.0 ** -ra), f32(2.0 ** -rb), f32(2.0 ** -pa), f16(f32(2.0 ** -pb))
    na = (sp.astype(np.float64) ** 2).sum(1).astype(f32)
    nb = (dp.astype(np.float64) ** 2).sum(1).astype(f32)
    n = len(sp)
    A, B = np.zeros((n, 32), f32), np.zeros((n, 32), f32)
    with np.errstate(over="ignore", invalid="ignore"):  # (a refused problem may pack infinities: nobody reads them)
        for base, pts, sign in ((0, sp, 1.0), (16, dp, -1.0)):
            for k in range(3):
                h, m, _ = split3(pts[:, k] * fra)
                A[:, base + 3 * k:base + 3 * k + 3] = np.stack([h, h, m], 1)
                h, m, _ = split3(pts[:, k] * frb)
                B[:, base + 3 * k:base + 3 * k + 3] = np.stack([f16(sign * 2 * h), f16(sign * 2 * m), f16(sign * 2 * h)], 1)
        h, m, l = split3(na * fpa)
        A[:, 9:12] = np.stack([-h, -m, -l], 1)
        B[:, 9:12] = P
        B[:, 12:15] = np.stack([-h, -m, -l], 1)
        A[:, 12:15] = P
        resid3 = float(np.abs((na * fpa).astype(np.float64) - h - m - l).max())
        h, m, l = split3(nb * fpa)
        A[:, 25:28] = np.stack([h, m, l], 1)
        B[:, 25:28] = P
        B[:, 28:31] = np.stack([h, m, l], 1)
        A[:, 28:31] = P
        resid3 = max(resid3, float(np.abs((nb * fpa).astype(np.float64) - h - m - l).max()))
    A[:, 31] = -0.25
    B[:, 31] = 1.0
    r2 = f32(max(na.max(), nb.max()))
    return A, B, r2, resid3


def operands_xy(src64, dst64, beta):
    g, kexp = scale2(beta)
    s = norm_shift(half_extent(src64, dst64))
    kexp += 2 * s
    gs = g * 2.0 ** s

    def centred(p):
        q = p.astype(f32)
        c = 0.5 * (q.min(0).astype(np.float64) + q.max(0).astype(np.float64))
        return ((p - c) * gs).astype(f32)

    sp, dp = centred(src64), centred(dst64)
    A, B, r2, resid3 = pack_xy(sp, dp, kexp)
    return dict(A=A, B=B, r2=r2, s=s, kexp=kexp, resid3=resid3, sp=sp, dp=dp)


def consts_xy(beta, s, r2):
    """k1c::consts_xy, step by step in f32"""
    g, kexp0 = scale2(beta)
    kexp = kexp0 + 2 * s
    beta_n = beta * g * 2.0 ** s
    up = f32(1.000001)
    r2 = f32(r2)
    with np.errstate(all="ignore"):
        b = f32(beta_n) * up
        kappa = f32(2.0 ** max(min(kexp, 1023), -1022))
        R2 = r2 * up
        R = np.sqrt(R2) * up
        b2 = f32(0.25) * kappa
        rng_ok = bool(R2 <= f32(8192)) and -17 <= kexp <= 15
        ra, rb, pa, pb = xy_shifts(kexp if rng_ok else 0)
        fra, frb, fpb = f32(2.0 ** -ra), f32(2.0 ** -rb), f32(2.0 ** -pb)
        sub_y = U * (R * (f32(6.1) * frb + f32(3.1) * fra) + f32(2) * fpb) * up
        eps_u = (K_EPS_Y * U * R2 + kappa * sub_y) * up
        eps_w = (kappa * (K_EPS_A * U * R2) + kappa * kappa * (f32(0.5) * sub_y)) * up
        lam_lo = f32(2) * f32(beta_n) * np.sqrt(r2) * f32(0.999999)
        lam_hi = f32(2) * b * R * up
        eta = eps_u / lam_lo * up
        ok = (bool(R2 > f32(1e-30)) and rng_ok and beta > 0 and bool(eta <= f32(0.125)) and bool(eta == eta) and
              bool(b2 * f32(5.76) <= R2) and bool(eps_w <= f32(0.004) * kappa * R2))
        den = f32(1) - f32(2) * (eta if ok else f32(0)) - f32(2) * U
        K2 = eta / den * up
        G = (f32(1.3e-13) * b * R2 * R + f32(8e-15) * b2 * R2) * up
        K0p = (eps_u * lam_hi + eps_u * eps_u + eps_w * (f32(1) + eta) + G) * up
        K0 = (K0p / den + f32(2) * K2 * eps_w) * up
        short_d = (f32(4) * b2 * b2 * (f32(1) + f32(16) * U) + f32(4) * b2 * eps_u + eps_u * eps_u + eps_w) * f32(1.001) * up
        K0e = K0 * f32(1.001) * up
        K0f = max(K0e, short_d) * f32(1.00001)
        U0 = (f32(4) * b * R * f32(1.001) + f32(2) * eps_u) * up
        E = (f32(2) * U0 * eps_u + eps_u * eps_u + eps_w + G) * up
        C0 = E / (f32(1) - f32(4) * U) * f32(1.001) * up
        C = max(C0, short_d) * f32(1.00001)
        ik = f32(2.0 ** (-kexp if rng_ok else 0))
        ik2 = ik * ik
        Cxy = C * ik2
        use = (ok and bool(K0f == K0f) and bool(K0f < f32(1e30)) and bool(short_d <= K_SHORT_RATIO * K0e) and bool(C == C) and
               bool(C < f32(1e30)) and bool(short_d <= K_SHORT_RATIO * C0) and bool(Cxy > 0) and bool(Cxy < f32(1e30)))
    return dict(C=Cxy, K2=K2 * f32(1.001) * up, K0=K0f * ik2, eps_y=eps_u * ik, eps_x=eps_w * ik2, kexp=kexp, use_mfma=int(use))


def filter_values_xy(op, i, j, rng):
    """(X~, Y~, d~ = fl(Y~^2 + X~)) of the pairs (i, j): the chain's first link accumulates slots 0..15 from zero, the
    second adds slots 16..31 onto it; several orders inside each link"""
    A, B = op["A"], op["B"]
    P = A[i].astype(np.float64) * B[j].astype(np.float64)  # exact: 11 x 11 bits
    assert (P.astype(f32) == P).all(), "a slot product is no exact f32"
    fma = lambda x, y, z: (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f32)
    orders = [(list(range(16)), list(range(16, 32))), (list(range(15, -1, -1)), list(range(31, 15, -1))),
              (list(rng.permutation(16)), list(16 + rng.permutation(16)))]
    out = []
    for o1, o2 in orders:
        X = accumulate(P, o1)
        Y = X.copy()
        for k in o2:
            Y = (Y + P[:, k].astype(f32)).astype(f32)
        out.append((X, Y, fma(Y, Y, X)))
    # worst case for the low bits: every pair adds the products of a link largest magnitude first
    P1, P2 = P[:, :16], P[:, 16:]
    s1 = np.take_along_axis(P1, np.argsort(-np.abs(P1), axis=1), axis=1)
    s2 = np.take_along_axis(P2, np.argsort(-np.abs(P2), axis=1), axis=1)
    X = accumulate(s1, range(16))
    Y = X.copy()
    for k in range(16):
        Y = (Y + s2[:, k].astype(f32)).astype(f32)
    out.append((X, Y, fma(Y, Y, X)))
    return out


def exact_xy(op, i, j):
    """X*, Y* of the normalised f32 points in double"""
    kappa = 2.0 ** op["kexp"]
    sp, dp = op["sp"].astype(np.float64), op["dp"].astype(np.float64)
    a = ((sp[j] - sp[i]) ** 2).sum(1)
    bb = ((dp[j] - dp[i]) ** 2).sum(1)
    return -a / kappa, (bb - a) / kappa - 0.25


def check(src, dst, beta, rng, npairs, pairs=None, admitted=True):
    n = len(src)
    op = operands_xy(src, dst, beta)
    kc = consts_xy(beta, op["s"], op["r2"])
    assert kc["use_mfma"] == int(admitted), "a test of a geometry that fell back to FP64 proves nothing"
    for M in (op["A"], op["B"]):
        assert np.isfinite(M).all() and np.abs(M).max() <= F16_MAX
        assert (M.astype(np.float16).astype(f32) == M).all()
    _, _, _, pb = xy_shifts(op["kexp"])
    assert op["resid3"] <= 2.0 ** -25  # the three pieces of a norm: exact, or short by half a subnormal step
    if pairs is None:
        i, j = rng.integers(0, n, size=npairs), rng.integers(0, n, size=npairs)
    else:
        i, j = pairs
    keep = i != j
    i, j = i[keep], j[keep]
    ref = reference_edge(src, dst, i, j, beta)
    Xs, Ys = exact_xy(op, i, j)
    frac = []
    for X, Y, d in filter_values_xy(op, i, j, rng):
        # the budget's two bounds themselves (the f32 rounding of the coordinates is part of them, not of X*, Y*,
        # which start from the rounded points: the bounds hold a fortiori)
        assert np.abs(X - Xs).max() <= kc["eps_x"] and np.abs(Y - Ys).max() <= kc["eps_y"]
        trusted = np.abs(d) > kc["C"]
        assert (np.signbit(d)[trusted] == ref[trusted]).all(), "the filter trusted a wrong sign"
        frac.append(trusted.mean())
    # self pairs: Y = -1/4, X = 0, d = 1/16 in exact arithmetic: never trusted
    k = np.arange(n)
    for _, _, d in filter_values_xy(op, k, k, rng):
        assert (np.abs(d) <= kc["C"]).all()
    return min(frac), op, kc


def test_xy_band_random_and_adversarial(capsys):
    rng = np.random.default_rng(2031)
    src, dst = bench_like(rng, 3000)
    frac, op, kc = check(src, dst, 0.02, rng, 300_000)
    frac_old, _, _ = old.check(src, dst, 0.02, np.random.default_rng(2031), 300_000)
    with capsys.disabled():
        print("\nbench-like cloud, beta = 0.02: in band %.3e of the pairs (X / Y), %.3e (u / w with a third MFMA); "
              "C = %.4g in units of Y^2 + X, kexp = %d" % (1 - frac, 1 - frac_old, float(kc["C"]), kc["kexp"]))
    assert frac > 0.998  # the filter decides almost everything
    # the budget's coefficient: 640 u R^2 / kappa plus the subnormal terms
    assert kc["eps_y"] * f32(2.0 ** kc["kexp"]) < f32(660.0) * U * op["r2"]
    for scale, nb in ((1.0, 0.01), (250.0, 0.05), (0.02, 1e-4)):
        src, dst = adversarial(rng, 1500, scale, 2 * nb)
        check(src, dst, 2 * nb, rng, 200_000)
    # large offsets are absorbed by the centring
    src = rng.uniform(size=(1000, 3)) + np.array([1e4, -2e4, 3e4])
    dst = src @ np.linalg.qr(rng.normal(size=(3, 3)))[0].T + 50.0
    check(src, dst, 0.02, rng, 100_000)
    # clouds of very different extent (|Y*| far beyond U0 / kappa for most pairs)
    src = rng.uniform(-1, 1, size=(1500, 3))
    dst = rng.uniform(-1, 1, size=(1500, 3)) * 0.05
    check(src, dst, 0.02, rng, 100_000)
    check(dst, src, 0.02, rng, 100_000)


def test_xy_band_subnormal_low_pieces():
    """one axis 1e-4 of the others: the low pieces of its coordinates are fp16 subnormals on both sides (absolute
    rounding error, the budget's sub_y / sub_x terms); a large beta (kexp > 0) pushes more pieces below 2^-14"""
    rng = np.random.default_rng(2032)
    src, dst = adversarial(rng, 1500, 1.0, 0.02, axes=(1.0, 1.0, 1e-4))
    _, op, _ = check(src, dst, 0.02, rng, 200_000)
    for M in (op["A"], op["B"]):
        m = np.abs(M[:, 8 if M is op["A"] else 7])  # m(s_z)
        assert ((m > 0) & (m < 2.0 ** -14)).mean() > 0.5
    src, dst = adversarial(rng, 1500, 1.0, 0.1, axes=(1.0, 1.0, 1e-3))
    _, op, kc = check(src, dst, 0.1, rng, 200_000)
    assert kc["kexp"] >= 4
    m = np.abs(op["A"][:, 8])
    assert ((m > 0) & (m < 2.0 ** -14)).mean() > 0.5


def test_xy_band_short_pairs_are_never_trusted():
    rng = np.random.default_rng(9)
    for scale, beta in ((1.0, 0.02), (1.0, 0.06), (1.0, 0.2), (10.0, 0.05), (0.05, 2e-4)):
        n = 1200
        centres = rng.uniform(-1, 1, size=(40, 3)) * scale
        which = rng.integers(0, 40, size=n)
        src = centres[which] + rng.uniform(-1, 1, size=(n, 3)) * beta * rng.choice([0.05, 0.3, 0.6], size=(n, 1))
        Rm = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        dst = src @ Rm.T + rng.uniform(-1, 1, size=(n, 3)) * beta * rng.choice([0.0, 0.05, 0.3], size=(n, 1))
        i = rng.integers(0, n, size=200_000)
        j = rng.integers(0, n, size=200_000)
        keep = (i != j) & (which[i] == which[j])
        i, j = i[keep], j[keep]
        _, op, kc = check(src, dst, beta, rng, 0, pairs=(i, j), admitted=beta != 0.2)
        a = np.linalg.norm(src[j] - src[i], axis=1)
        b = np.linalg.norm(dst[j] - dst[i], axis=1)
        short = a + b <= beta * (1 + 1e-9)
        assert short.sum() > 500
        for _, _, d in filter_values_xy(op, i, j, rng):
            assert not (np.abs(d) > kc["C"])[short].any()


def test_xy_power_of_two_rescaling_packs_the_same_bits():
    rng = np.random.default_rng(2033)
    src, dst = bench_like(rng, 500)
    ref = operands_xy(src, dst, 0.02)
    kc = consts_xy(0.02, ref["s"], ref["r2"])
    for k in (-20, -8, -6, 6, 8, 20):
        f = 2.0 ** k
        op = operands_xy(src * f, dst * f, 0.02 * f)
        assert op["s"] == ref["s"] - k and op["kexp"] == ref["kexp"]
        assert (op["A"] == ref["A"]).all() and (op["B"] == ref["B"]).all() and op["r2"] == ref["r2"]
        assert consts_xy(0.02 * f, op["s"], op["r2"]) == kc


def admitted_interval(src, dst):
    """the smallest and the largest admitted beta of a cloud (bisection on the admission test), and their neighbours
    just outside"""
    def adm(beta):
        op = operands_xy(src, dst, beta)
        return consts_xy(beta, op["s"], op["r2"])["use_mfma"] == 1

    assert adm(0.02)
    ends = []
    for out in (1e-6, 0.9):
        lo, hi = 0.02, out  # lo admitted, hi refused
        assert not adm(hi)
        for _ in range(40):
            mid = math.sqrt(lo * hi)
            lo, hi = (mid, hi) if adm(mid) else (lo, mid)
        ends.append((lo, hi))
    return ends


def test_xy_admission_boundaries():
    rng = np.random.default_rng(2034)
    src, dst = bench_like(rng, 1500)
    (b_lo, b_lo_out), (b_hi, b_hi_out) = admitted_interval(src, dst)
    # the lower end is the eta <= 1/8 condition: R / beta ~ 2^24 / (8 x 320) = 6550 in the normalised system; the upper
    # end the short-pair limit, beta ~ 0.1 R
    for beta, inside in ((b_lo, True), (b_lo_out, False), (b_hi, True), (b_hi_out, False)):
        op = operands_xy(src, dst, beta)
        kc = consts_xy(beta, op["s"], op["r2"])
        assert kc["use_mfma"] == int(inside)
    def r_over_beta(beta):  # in the normalised system
        op = operands_xy(src, dst, beta)
        return math.sqrt(float(op["r2"])) / (beta * scale2(beta)[0] * 2.0 ** op["s"])

    assert 5500 < r_over_beta(b_lo) < 6600 and 0.05 < 1 / r_over_beta(b_hi) < 0.2
    # at both ends the band holds (the band is checked whether or not the problem is admitted: just outside too)
    check(src, dst, b_lo, rng, 200_000)
    check(src, dst, b_hi, rng, 200_000)
    check(src, dst, b_lo_out, rng, 100_000, admitted=False)
    # everything consts() admits of the GPU tests' geometries is admitted here as well: the bench cloud and its
    # rescalings, the adversarial clouds (test_xy_band_random_and_adversarial), the shrunk cloud of the mixed batch
    for k in (-20, -8, 0, 8, 20):
        op = operands_xy(src * 2.0 ** k, dst * 2.0 ** k, 0.02 * 2.0 ** k)
        assert consts_xy(0.02 * 2.0 ** k, op["s"], op["r2"])["use_mfma"] == 1
    op = operands_xy(src * 2.0 ** -13, dst * 2.0 ** -13, 2e-7)
    assert consts_xy(2e-7, op["s"], op["r2"])["use_mfma"] == old.consts(2e-7, op["s"], op["r2"])["use_mfma"] == 1
    # refused: beta far below the resolution, beta of the size of the cloud, a box that says nothing about the points
    op = operands_xy(src, dst, 2e-7)
    assert consts_xy(2e-7, op["s"], op["r2"])["use_mfma"] == 0
    op = operands_xy(src, dst, 0.9)
    assert consts_xy(0.9, op["s"], op["r2"])["use_mfma"] == 0
    with np.errstate(all="ignore"):
        op = operands_xy(src + 1e12, dst, 0.02)
    assert consts_xy(0.02, op["s"], op["r2"])["use_mfma"] == 0
    # the range conditions by themselves: kexp outside [-17, 15], R^2 above 8192, no finite R^2, beta = 0
    for beta, s, r2 in ((2.0 ** -10, 0, f32(300.0)), (2.0 ** 8, 0, f32(300.0)), (0.7, 0, f32(8200.0)),
                        (0.7, 0, f32(np.inf)), (0.7, 0, f32(np.nan)), (0.0, 0, f32(3000.0))):
        assert consts_xy(beta, s, r2)["use_mfma"] == 0


def test_xy_fp16_range_at_the_ends_of_the_kexp_window():
    """points on the rim of the admitted window (R^2 just below 8192, coordinates up to 90.5) at kexp = -17 and 15: every
    piece is a finite fp16 value, and at kexp = -17 the largest ones stand where the header puts them"""
    rng = np.random.default_rng(2035)
    d = rng.normal(size=(400, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:3] = np.eye(3)
    pts = (d * 90.5).astype(f32)
    for kexp in (-17, -16, -3, -2, -1, 0, 1, 15):
        A, B, r2, resid3 = pack_xy(pts, pts[::-1].copy(), kexp)
        assert r2 <= 8192
        for M in (A, B):
            assert np.isfinite(M).all() and np.abs(M).max() <= F16_MAX
            assert (M.astype(np.float16).astype(f32) == M).all()
        assert resid3 <= 2.0 ** -25
    A, B, _, _ = pack_xy(pts, pts, -17)
    assert np.abs(A[:, :9]).max() == 90.5 * 512 and np.abs(B[:, :9]).max() == 2 * 90.5 * 256 and B[0, 9] == 2.0 ** 15
