"""Inputs of the estimator edge tests (tests/test_estimator_cases.py on the CPU, tests/test_gpu_estimator_edges.py on the
GPU): correspondences whose clique size is chosen, not found.  With use_max_clique = False the clique is 0 .. n - 1
(effective_mode() in csrc/solver.hip, mode 3 in the oracle), so K = n exactly and the content of the "clique" -- gross
outliers included -- is the test's to choose.  numpy only; every array is a function of (K, kind, seed, scale, offset).

    SIZES   what the size exercises in csrc/kernels_estimate.hip
    2       one distinct TIM
    3       the smallest size with a determined R
    8 / 9   lane 0 of the register sort full, lane 1 begins
    63..65  wave edge of the gather and of the compaction
    255..258  slot 0 of the fast route full; slot 1's first and second element; the wrap TIM sits in slot 1
    511 / 512  last padded lane of the sort, then no padding plus the p1[K] special case
    513     first clique on the general route
    1024 / 1025  endpoint sort in LDS, then in global scratch (kTlsLdsEndpoints = 2048 = 2 K)
"""
import numpy as np

NB = 0.01  # noise bound of every case
SIZES = (2, 3, 8, 9, 63, 64, 65, 255, 256, 257, 258, 511, 512, 513, 1024, 1025)
KINDS = ("clean", "rigid", "outliers", "dups", "singletons")
SINGLETON_STEP = 3 * NB  # per-axis distance of neighbouring translation residuals (> 2 beta = 2 NB)


def random_rotation(rng):
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    return Q


def yaw_rotation(rng):
    th = rng.uniform(-np.pi, np.pi)
    return np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])


def ball(rng, radius, K):
    """K points uniform in the ball of `radius`, 3 x K"""
    v = rng.normal(size=(3, K))
    v /= np.linalg.norm(v, axis=0)
    return v * (radius * rng.uniform(size=K) ** (1.0 / 3.0))


def case(K, kind, seed, scale=1.0, offset=1.0, yaw_only=False):
    """dict(src 3 x K, dst 3 x K, R, t, scale, outliers): dst = scale R src + t + e, e by `kind`:
    clean       e uniform in a ball of radius 0.6 NB: every TIM residual is below the rotation bound 2 NB, GNC-TLS
                breaks in its first iteration (mu <= 0: cost = inf, iterations = 1)
    rigid       e = 0
    outliers    clean, then max(1, K // 5) columns of dst are scale U(-1, 1)^3 + t   (K >= 8)
    dups        outliers, then columns K // 2 .. 2 (K // 2) - 1 of BOTH clouds are exact copies of columns
                0 .. K // 2 - 1: exactly equal values in the translation sort   (scale = 1 only: the scale estimate of
                duplicated points is ill-posed)
    singletons  R = I, dst = src + t + SINGLETON_STEP j (1, 1, 1) with src scaled to 5e-4 and t in [4, 4.05]^3: per
                axis the translation residuals are pairwise more than 2 beta apart, every consensus set has one member
    yaw_only: R is a rotation about z (what QUATRO estimates)."""
    if kind not in KINDS:
        raise ValueError(kind)
    if kind in ("outliers", "dups") and K < 8:
        raise ValueError("%s needs K >= 8" % kind)
    if kind in ("dups", "singletons") and scale != 1.0:
        raise ValueError("%s is not combined with a scale" % kind)
    rng = np.random.default_rng([int(seed), int(K), KINDS.index(kind)])
    src = rng.uniform(-1, 1, size=(3, K))
    R = yaw_rotation(rng) if yaw_only else random_rotation(rng)
    t = offset * rng.uniform(-1, 1, size=3)
    e = ball(rng, 0.6 * NB, K)
    bad = np.zeros(K, dtype=bool)
    if kind == "singletons":
        # Every consecutive TIM is off by SINGLETON_STEP (1, 1, 1), more than the rotation bound, so the estimated R is
        # whatever GNC-TLS leaves when all weights reach 0: src is small (5e-4) so that the residuals dst - R src stay
        # singletons, smallest at column 0, under ANY rotation.  t lies in [4, 4.05]^3, so that up to K = 64 the values
        # lie in [4, 6.4): for a mantissa below 1.6 the reference's x_hat = (x w) / w with w = 1 / beta^2 is x exactly
        # (the mantissa of the rounded product x w is 1.22 times that of x, so its rounding error, divided by w, is
        # below half an ulp of x) and its residual x_hat^2 + x^2 - 2 x x_hat exactly 0.  Elsewhere x_hat can be one
        # ulp off, the residual +-1e-17, and the reference's own choice among the (equally good) singletons a matter
        # of rounding: tests/test_fused_translation_model.py records that.
        R = np.eye(3)
        src = 5e-4 * src
        t = offset * (4.0 + 0.05 * rng.uniform(size=3))
        dst = src + t[:, None] + SINGLETON_STEP * np.arange(K)[None, :] * np.ones((3, 1))
        return dict(src=src, dst=dst, R=R, t=t, scale=1.0, outliers=bad)
    dst = scale * (R @ src) + t[:, None]
    if kind != "rigid":
        dst = dst + e
    if kind in ("outliers", "dups"):
        m = max(1, K // 5)
        cols = rng.choice(K, size=m, replace=False)
        dst[:, cols] = scale * rng.uniform(-1, 1, size=(3, m)) + t[:, None]
        bad[cols] = True
    if kind == "dups":
        h = K // 2
        src[:, h:2 * h] = src[:, :h]
        dst[:, h:2 * h] = dst[:, :h]
        bad[h:2 * h] = bad[:h]
    return dict(src=src, dst=dst, R=R, t=t, scale=float(scale), outliers=bad)


def chain_tims(p):
    """3 x K chain TIMs of a 3 x K cloud: TIM j = vertex (j + 1) % K minus vertex j (registration.cc:657-680)"""
    return np.roll(p, -1, axis=1) - p


def params(**kw):
    """the benchmark's solver parameters with the clique switched off (K = n) and a tight GNC stop"""
    p = dict(noise_bound=NB, cbar2=1.0, estimate_scaling=False, rotation_gnc_factor=1.4, rotation_max_iterations=100,
             rotation_cost_threshold=1e-12, use_max_clique=False)
    p.update(kw)
    return p


def oracle_kw(p):
    """the oracle's spelling of `params` (integers for the enumerations and flags)"""
    q = dict(p)
    for k in ("estimate_scaling", "use_max_clique", "rotation_estimation_algorithm", "rotation_tim_graph"):
        if k in q:
            q[k] = int(q[k])
    return q


# ---------------------------------------------------------------------------------------------------------------------
# The solves of the GPU tests, as (id, case arguments, parameter overrides): tests/test_estimator_cases.py holds the
# oracle alone to the conditions the GPU tolerances rest on for exactly this list.
# ---------------------------------------------------------------------------------------------------------------------
SEED = 7100
SUBSET = (3, 257, 512, 513)            # sizes that also run at the benchmark threshold, far from the origin and scaled
OTHER_SIZES = (3, 255, 256, 257, 513)  # FGR / QUATRO
COMPLETE_SIZES = (3, 23, 24, 65)       # KT = 3, 253, 276, 2080: the TIM count crosses one block between 23 and 24
FGR, QUATRO = 1, 2
COMPLETE = 1


def kind_at(K, kind):
    """`outliers` and `dups` exist from K = 8 on; below, the case is `clean`"""
    return kind if K >= 8 else "clean"


def solve_cases():
    out = []
    for K in SIZES:
        if K < 3:
            continue
        for kind in ("clean", "outliers", "dups"):
            if K < 8 and kind != "clean":
                continue
            out.append(("route-%d-%s" % (K, kind), dict(K=K, kind=kind, seed=SEED), {}))
    for K in SUBSET:
        for kind in ("clean", "outliers", "dups"):
            if K < 8 and kind != "clean":
                continue
            out.append(("bench-threshold-%d-%s" % (K, kind), dict(K=K, kind=kind, seed=SEED + 1),
                        dict(rotation_cost_threshold=0.005)))
            out.append(("offset-%d-%s" % (K, kind), dict(K=K, kind=kind, seed=SEED + 2, offset=1000.0), {}))
        for kind in ("clean", "outliers"):
            if K < 8 and kind != "clean":
                continue
            out.append(("scaled-%d-%s" % (K, kind), dict(K=K, kind=kind, seed=SEED + 3, scale=1.7),
                        dict(estimate_scaling=True)))
    for K in OTHER_SIZES:
        out.append(("fgr-%d" % K, dict(K=K, kind=kind_at(K, "outliers"), seed=SEED + 4),
                    dict(rotation_estimation_algorithm=FGR)))
        out.append(("quatro-%d" % K, dict(K=K, kind=kind_at(K, "outliers"), seed=SEED + 5, yaw_only=True),
                    dict(rotation_estimation_algorithm=QUATRO)))
    for K in COMPLETE_SIZES:
        out.append(("complete-%d" % K, dict(K=K, kind=kind_at(K, "outliers"), seed=SEED + 6),
                    dict(rotation_tim_graph=COMPLETE)))
    return out


SINGLETON_SOLVE_SIZES = (2, 3, 5)
SINGLETON_STAGE_SIZES = (2, 3, 5, 64)

# Exact endpoint ties that do NOT leave the answer open: src = 0 (so dst - R src = dst under any R), beta = 1, values on a
# grid of 1 / 4 with members exactly 2 beta apart.  On each axis the optimal consensus set is a window (x_i, x_i + 2 beta]
# right after the closing of x_i, with a member exactly at x_i + 2 beta: the reference evaluates it in either order of the
# tied endpoints, and a closing search that drops the tied opening (< for <=) evaluates it nowhere.
TIE_NB = 1.0
TIE_DST = np.array([[4.0, 3.5, 1.0, 2.0], [2.25, 8.25, 2.5, 0.5], [3.5, 5.0, 5.5, 5.0]])
