"""CPU model of the K1 filter on two-piece fp16 operands (csrc/kernels_graph.hip, csrc/k1_consts.h).

A numpy re-implementation of the pre-pass (centring, the scale g, the power-of-two normalisation, f32 rounding, the
fp16 splits with subnormal rounding, the K-slot table), of the band constants and the admission test, and of an f32
accumulation under the documented hardware model (exact products, every addition rounded to f32; several orders,
among them largest-magnitude-first, which loses the most low bits).  It pins the slot table and the constants: a
pair the constant band trusts must get the reference's answer, short pairs and self pairs are never trusted, and
every packed piece of an admitted problem is a finite fp16 value.  (The GPU tests check the real instruction.)"""
import math

import numpy as np

from test_k1_band_model import reference_edge

f32 = np.float32
U = f32(2.0 ** -24)
K_EPS_U = f32(500.0)
K_EPS_A = f32(200.0)
K_SHORT_RATIO = f32(21.76)
F16_MAX = 65504.0


def scale2(beta):
    """g in (1, sqrt 2], kexp: 4 (g beta)^2 = 2^kexp"""
    x = 4.0 * beta * beta
    if not (1e-300 < x < 1e300):
        return 1.0, 0
    kexp = math.frexp(x)[1]  # floor(log2 x) + 1
    return math.sqrt(2.0 ** kexp / x), kexp


def norm_shift(H):
    if not (1e-280 < H < 1e280):
        return 0
    return 4 - (math.frexp(H)[1] - 1)


def f16(v):
    with np.errstate(over="ignore"):
        return np.asarray(v, f32).astype(np.float16).astype(f32)


def split3(v):
    v = np.asarray(v, f32)
    h = f16(v)
    r1 = (v - h).astype(f32)
    m = f16(r1)
    return h, m, f16((r1 - m).astype(f32))


def half_extent(src64, dst64):
    H = 0.0
    for p in (src64, dst64):
        q = p.astype(f32).astype(np.float64)
        H = max(H, float((0.5 * (q.max(0) - q.min(0))).max()))
    return H


def operands(src64, dst64, beta):
    """per point: row side A [n, 48] (slots 0..31 the u chain, 32..47 the w MFMA), column side B [n, 32] (the w MFMA
    runs over B[:, 0:16] again), as f32 arrays of fp16-representable values; R^2 (f32), the shift s, kexp (normalised)"""
    g, kexp = scale2(beta)
    s = norm_shift(half_extent(src64, dst64))
    kexp += 2 * s
    gs = g * 2.0 ** s
    kappa = f32(2.0 ** kexp)

    def centred(p):
        q = p.astype(f32)
        c = 0.5 * (q.min(0).astype(np.float64) + q.max(0).astype(np.float64))
        return ((p - c) * gs).astype(f32)

    sp, dp = centred(src64), centred(dst64)
    na = (sp.astype(np.float64) ** 2).sum(1)
    nb = (dp.astype(np.float64) ** 2).sum(1)
    n = len(sp)
    A, B = np.zeros((n, 48), f32), np.zeros((n, 32), f32)
    resid = 0.0  # max of |v - h - m| / max(2^-22 |v|, 2^-25) over the coordinates
    for k in range(3):
        h, m, _ = split3(sp[:, k])
        resid = max(resid, float((np.abs(sp[:, k].astype(np.float64) - h - m) /
                                  np.maximum(2.0 ** -22 * np.abs(sp[:, k]), 2.0 ** -25)).max()))
        A[:, 3 * k:3 * k + 3] = np.stack([h, h, m], 1)
        B[:, 3 * k:3 * k + 3] = np.stack([f16(2 * h), f16(2 * m), f16(2 * h)], 1)
        A[:, 32 + 3 * k:32 + 3 * k + 3] = np.stack([f16(kappa * h), f16(kappa * h), f16(kappa * m)], 1)
        h, m, _ = split3(dp[:, k])
        resid = max(resid, float((np.abs(dp[:, k].astype(np.float64) - h - m) /
                                  np.maximum(2.0 ** -22 * np.abs(dp[:, k]), 2.0 ** -25)).max()))
        A[:, 16 + 3 * k:16 + 3 * k + 3] = np.stack([h, h, m], 1)
        B[:, 16 + 3 * k:16 + 3 * k + 3] = np.stack([f16(-2 * h), f16(-2 * m), f16(-2 * h)], 1)
    beta2s = 2.0 ** (kexp - 2)
    h, m, _ = split3(na.astype(f32))
    B[:, 9:11] = np.stack([-h, -m], 1)
    A[:, 32 + 9:32 + 11] = f16(kappa)
    B[:, 11:14] = 1
    B[:, 14:16] = f16(kappa)
    A[:, 32 + 14:32 + 16] = np.stack([-h, -m], 1)
    drow, dcol = (nb - na - beta2s).astype(f32), (nb - na).astype(f32)
    h, m, l = split3(drow)
    A[:, 11:14] = np.stack([h, m, l], 1)
    resid3 = float(np.abs(drow.astype(np.float64) - h - m - l).max())
    h, m, l = split3(dcol)
    A[:, 25:28] = 1
    B[:, 25:28] = np.stack([h, m, l], 1)
    resid3 = max(resid3, float(np.abs(dcol.astype(np.float64) - h - m - l).max()))
    r2 = f32(max(na.astype(f32).max(), nb.astype(f32).max()))
    return dict(A=A, B=B, r2=r2, s=s, kexp=kexp, resid=resid, resid3=resid3)


def consts(beta, s, r2):
    """k1c::consts, step by step in f32"""
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
        eps_u = (K_EPS_U * U * R2 + U * (f32(12.1) * R + f32(1))) * up
        eps_w = (kappa * (K_EPS_A * U * R2) + U * (f32(6.1) * R + kappa * (f32(3.1) * R + f32(1)))) * up
        lam_lo = f32(2) * f32(beta_n) * np.sqrt(r2) * f32(0.999999)
        lam_hi = f32(2) * b * R * up
        eta = eps_u / lam_lo * up
        rng_ok = bool(R2 <= f32(8192)) and -24 <= kexp <= 15 and bool(kappa * R * f32(1.001) <= f32(60000))
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
        use = (ok and bool(K0f == K0f) and bool(K0f < f32(1e30)) and bool(short_d <= K_SHORT_RATIO * K0e) and bool(C == C) and
               bool(C < f32(1e30)) and bool(short_d <= K_SHORT_RATIO * C0))
    return dict(C=C, K2=K2 * f32(1.001) * up, K0=K0f, eps_u=eps_u, eps_w=eps_w, kexp=kexp, use_mfma=int(use))


def accumulate(P, order):
    """sum of the exact products P[:, k] in the given order, every addition rounded to f32"""
    acc = np.zeros(P.shape[0], f32)
    for k in order:
        acc = (acc + P[:, k].astype(f32)).astype(f32)
    return acc


def filter_values(op, i, j, rng):
    """d~ of the pairs (i, j) under several accumulation orders"""
    A, B = op["A"], op["B"]
    Pu = A[i, :32].astype(np.float64) * B[j].astype(np.float64)      # exact: 11 x 11 bits
    Pw = A[i, 32:].astype(np.float64) * B[j, :16].astype(np.float64)
    assert (Pu.astype(f32) == Pu).all() and (Pw.astype(f32) == Pw).all()
    fma = lambda x, y, z: (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f32)
    out = []
    chain = [list(range(32)), list(range(31, -1, -1)),
             list(rng.permutation(16)) + list(16 + rng.permutation(16))]
    for ou in chain:
        ow = [k for k in ou if k < 16]
        u, w = accumulate(Pu, ou), accumulate(Pw, ow)
        out.append(fma(u, u, w))
    # worst case for the low bits: every pair adds its own products largest magnitude first
    su = np.take_along_axis(Pu, np.argsort(-np.abs(Pu), axis=1), axis=1)
    sw = np.take_along_axis(Pw, np.argsort(-np.abs(Pw), axis=1), axis=1)
    u, w = accumulate(su, range(32)), accumulate(sw, range(16))
    out.append(fma(u, u, w))
    return out


def check(src, dst, beta, rng, npairs, pairs=None, admitted=True):
    n = len(src)
    op = operands(src, dst, beta)
    kc = consts(beta, op["s"], op["r2"])
    assert kc["use_mfma"] == int(admitted), "a test of a geometry that fell back to FP64 proves nothing"
    # every packed piece is a finite fp16 value, and the split residuals are what the budget assumes
    for M in (op["A"], op["B"]):
        assert np.isfinite(M).all() and np.abs(M).max() <= F16_MAX
        assert (M.astype(np.float16).astype(f32) == M).all()
    assert op["resid"] <= 1.0 and op["resid3"] <= 2.0 ** -25
    if pairs is None:
        i, j = rng.integers(0, n, size=npairs), rng.integers(0, n, size=npairs)
    else:
        i, j = pairs
    keep = i != j
    i, j = i[keep], j[keep]
    ref = reference_edge(src, dst, i, j, beta)
    frac = []
    for d in filter_values(op, i, j, rng):
        trusted = np.abs(d) > kc["C"]
        assert (np.signbit(d)[trusted] == ref[trusted]).all(), "the filter trusted a wrong sign"
        frac.append(trusted.mean())
    # self pairs: u = -beta^2, w = 0 exactly in exact arithmetic, d = beta^4 <= C: never trusted
    k = np.arange(n)
    for d in filter_values(op, k, k, rng):
        assert (np.abs(d) <= kc["C"]).all()
    return min(frac), op, kc


def bench_like(rng, n):
    src = rng.uniform(size=(n, 3))
    Rm = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    dst = src @ Rm.T + rng.uniform(-1, 1, size=3)
    out = rng.uniform(size=n) < 0.95
    dst[out] = rng.uniform(-1, 1, size=(int(out.sum()), 3))
    dst[~out] += rng.uniform(-0.0057, 0.0057, size=(int((~out).sum()), 3))
    return src, dst


def adversarial(rng, n, scale, beta, axes=(1.0, 1.0, 1.0)):
    """pairs engineered onto the boundary: dst lengths = src lengths +- beta (1 + delta)"""
    src = rng.uniform(-1, 1, size=(n, 3)) * scale * np.asarray(axes)
    Rm = np.linalg.qr(rng.normal(size=(3, 3)))[0] if axes == (1.0, 1.0, 1.0) else np.eye(3)
    dst = src @ Rm.T
    off = rng.choice([0.0, 1.0, -1.0], size=n) * beta * (
        1 + rng.choice([0, 1e-15, 1e-12, 1e-9, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3], size=n))
    d = dst / np.linalg.norm(dst, axis=1, keepdims=True)
    return src, dst + d * (off * rng.uniform(0.3, 1.0, size=n))[:, None]


def test_f16_band_random_and_adversarial():
    rng = np.random.default_rng(2031)
    src, dst = bench_like(rng, 3000)
    frac, _, _ = check(src, dst, 0.02, rng, 300_000)
    assert frac > 0.998  # the filter decides almost everything
    # the three scales of test_k1_filter_adversarial_band (beta = 2 nb)
    for scale, nb in ((1.0, 0.01), (250.0, 0.05), (0.02, 1e-4)):
        src, dst = adversarial(rng, 1500, scale, 2 * nb)
        check(src, dst, 2 * nb, rng, 200_000)
    # large offsets are absorbed by the centring
    src = rng.uniform(size=(1000, 3)) + np.array([1e4, -2e4, 3e4])
    dst = src @ np.linalg.qr(rng.normal(size=(3, 3)))[0].T + 50.0
    check(src, dst, 0.02, rng, 100_000)
    # clouds of very different extent (|u*| far beyond U0 for most pairs)
    src = rng.uniform(-1, 1, size=(1500, 3))
    dst = rng.uniform(-1, 1, size=(1500, 3)) * 0.05
    check(src, dst, 0.02, rng, 100_000)
    check(dst, src, 0.02, rng, 100_000)


def test_f16_band_subnormal_low_pieces():
    """one axis 1e-4 of the others: its coordinates are ~2^-8 in the normalised system, their low pieces fp16
    subnormals (absolute rounding error, the budget's sub_u / sub_w terms)"""
    rng = np.random.default_rng(2032)
    src, dst = adversarial(rng, 1500, 1.0, 0.02, axes=(1.0, 1.0, 1e-4))
    _, op, _ = check(src, dst, 0.02, rng, 200_000)
    m = np.abs(op["A"][:, 8])  # m(s_z)
    assert ((m > 0) & (m < 2.0 ** -14)).mean() > 0.5


def test_f16_band_short_pairs_are_never_trusted():
    rng = np.random.default_rng(9)
    # (beta = 0.2 on a unit cloud: 4 beta^4 is 31 x the error term, the admission test sends it to FP64 -- the band
    # must hold all the same)
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
        for d in filter_values(op, i, j, rng):
            assert not (np.abs(d) > kc["C"])[short].any()


def test_f16_power_of_two_rescaling_packs_the_same_bits():
    rng = np.random.default_rng(2033)
    src, dst = bench_like(rng, 500)
    ref = operands(src, dst, 0.02)
    kc = consts(0.02, ref["s"], ref["r2"])
    for k in (-20, -8, 8, 20):
        f = 2.0 ** k
        op = operands(src * f, dst * f, 0.02 * f)
        assert op["s"] == ref["s"] - k and op["kexp"] == ref["kexp"]
        assert (op["A"] == ref["A"]).all() and (op["B"] == ref["B"]).all() and op["r2"] == ref["r2"]
        assert consts(0.02 * f, op["s"], op["r2"]) == kc


def test_f16_admission():
    rng = np.random.default_rng(2034)
    src, dst = bench_like(rng, 500)
    op = operands(src, dst, 2e-7)  # beta far below the filter's resolution
    assert consts(2e-7, op["s"], op["r2"])["use_mfma"] == 0
    op = operands(src, dst, 0.9)   # beta of the size of the cloud
    assert consts(0.9, op["s"], op["r2"])["use_mfma"] == 0
    # a bounding box that says nothing about the points (offsets beyond f32's resolution): R^2 decides
    far = src + 1e12
    with np.errstate(all="ignore"):
        op = operands(far, dst, 0.02)
    assert consts(0.02, op["s"], op["r2"])["use_mfma"] == 0
    # the error budget's terms against the issue's sketch: the band must be narrower than the bf16 formulation's
    op = operands(src, dst, 0.02)
    kc = consts(0.02, op["s"], op["r2"])
    assert kc["use_mfma"] == 1 and kc["eps_u"] < f32(520.0) * U * op["r2"]
