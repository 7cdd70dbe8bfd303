#!/usr/bin/env python3
"""Generates tests/golden/ransac_golden.npz: the inputs of the RANSAC tests and, per trial, what the estimate must be.

Trial cases (2 048 trials each, points on the 1/1024 dyadic grid, P in [-1, 1]^3):
  e3, e255   a 90 degree rotation about z and a dyadic translation: the planted inliers are exact
  n48, n256, n257   a general pose and Gaussian noise of 0.003 on the planted inliers (rounded to the grid)
  tiny2      ncorr = 2 < ransac_n: nothing is drawn
n256 samples four pairs per trial, the others three.  The pairs are shuffled, some repeat, and the clouds hold more
points than the pairs use.  Per trial the fixture holds the Kabsch pose of its samples from the exact sums at 50 digits
(tests/icp_step_reference.umeyama_step, rounded to FP64; the 12 entries of [R | t]), its conditioning
s0 / (s1 + d s2) (inf where the rotation is not unique: rank(H) <= 1) and A, the Frobenius error of the numpy
restatement (tests/ransac_reference.estimate) against it.  cond and A are stored as float32: the bar built from them
moves by 6e-8 of itself.
Asserted here, on the CPU: at most a quarter of the trials of a case with ncorr >= 48 have cond > 1e3 (e3 cannot meet
that: three draws with replacement from three pairs repeat a pair in 21 of 27 cases; its 27 sample triples are all
there is to check).  Printed, not asserted: how A compares with 16 * 2^-52 cond (four samples with a near-reflective
H put the numpy SVD a few times above it; A is in the bar for that).
Loop cases: `early` stops by the confidence rule strictly between two multiples of 64 after more than 64 trials;
`full` runs to max_iteration.  Both behaviours are asserted here with the restatement.
Needs mpmath.  Run from the repo root (CPU only, a few minutes):  python tests/golden/make_ransac_golden.py"""
import os
import sys
from fractions import Fraction as Fr

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_step_reference as S  # noqa: E402
import ransac_reference as RR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ransac_golden.npz")
TRIALS = 2048
COND_MAX = 1e3
GRID = 1024.0
R_MATCH = 1.0 / 64


def grid(a):
    return np.round(np.asarray(a) * GRID) / GRID


def pose_exact():
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [0.25, -0.5, 0.125]
    return T


def pose_general(rng):
    w = rng.normal(size=3)
    w *= 0.9 / np.linalg.norm(w)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = [0.3, -0.2, 0.1]
    return T


def make_case(seed, ncorr, n_inl, exact, ransac_n=3, s=0.9, d=1.0 / 32, noise=0.003):
    rng = np.random.default_rng(seed)
    extra = 5 if ncorr > 3 else 0
    n_s, n_t = ncorr + extra, ncorr + extra + 2
    P = rng.integers(-1024, 1025, size=(n_s, 3)) / GRID
    T = pose_exact() if exact else pose_general(rng)
    Q = rng.integers(-1024, 1025, size=(n_t, 3)) / GRID
    src = rng.permutation(n_s)[:ncorr]
    dst = rng.permutation(n_t)[:ncorr]
    planted = np.zeros(ncorr, dtype=bool)
    planted[rng.permutation(ncorr)[:n_inl]] = True
    moved = P[src] @ T[:3, :3].T + T[:3, 3]
    if not exact:
        moved = grid(moved + rng.normal(scale=noise, size=moved.shape))
    Q[dst[planted]] = moved[planted]
    corr = np.stack([src, dst], 1).astype(np.int32)
    if ncorr >= 48:  # repeats: the last two pairs repeat the first two
        corr[-2:] = corr[:2]
        planted[-2:] = planted[:2]
    return dict(P=P, Q=Q, corr=corr, planted=planted, T_true=T, ransac_n=ransac_n,
                params=np.array([R_MATCH, s, d]), seed=np.array([0x5EED0000 + seed], dtype=np.uint64))


def exact_step(ctx, rec, smp_row):
    f = [[Fr(float(v)) for v in rec[k]] for k in smp_row]
    s = dict(cnt=len(f), centre=[Fr(0)] * 3,
             sp=[sum(r[a] for r in f) for a in range(3)], sq=[sum(r[3 + a] for r in f) for a in range(3)],
             spq=[[sum(r[a] * r[3 + b] for r in f) for b in range(3)] for a in range(3)])
    u = S.umeyama_step(ctx, s)
    if not u["unique"]:
        return np.eye(4)[:3].ravel(), np.inf
    return np.array([[float(u["U"][r, c]) for c in range(4)] for r in range(3)]).ravel(), u["cond"]


def per_trial(ctx, c):
    ncorr, n = len(c["corr"]), c["ransac_n"]
    rec = RR.records_of(c["P"], c["Q"], c["corr"])
    smp = RR.samples(int(c["seed"][0]), n, ncorr, 0, TRIALS)
    gT, cond, A = np.zeros((TRIALS, 12)), np.zeros(TRIALS, np.float32), np.zeros(TRIALS, np.float32)
    cache = {}
    for q in range(TRIALS):
        key = tuple(smp[q])
        if key not in cache:
            T, cd = exact_step(ctx, rec, smp[q])
            a = np.linalg.norm(RR.estimate(rec, smp[q])[:3].ravel() - T) if np.isfinite(cd) else 0.0
            cache[key] = (T, np.float32(cd), np.float32(a))
        gT[q], cond[q], A[q] = cache[key]
    return gT, cond, A


def main():
    ctx = S.context()
    cases = dict(e3=make_case(1, 3, 3, True), n48=make_case(2, 48, 24, False), e255=make_case(3, 255, 128, True),
                 n256=make_case(4, 256, 160, False, ransac_n=4), n257=make_case(5, 257, 128, False),
                 tiny2=make_case(6, 2, 2, True))
    d = dict(trial_cases=np.array(["e3", "n48", "e255", "n256", "n257"]), trials=np.array(TRIALS))
    for name, c in cases.items():
        for k in ("P", "Q", "corr", "planted", "T_true", "params", "seed"):
            d[name + "/" + k] = c[k]
        d[name + "/ransac_n"] = np.array(c["ransac_n"])
        if name == "tiny2":
            continue
        gT, cond, A = per_trial(ctx, c)
        d[name + "/gT"], d[name + "/cond"], d[name + "/A"] = gT, cond, A
        good = cond <= COND_MAX
        left_out = 1.0 - good.mean()
        worst = float((A[good].astype(np.float64) / (16 * 2.0 ** -52 * cond[good].astype(np.float64))).max())
        print("%-5s ncorr %3d  cond > 1e3 or not unique: %5.1f %%   max A / (16 2^-52 cond) = %.3g" % (
            name, len(c["corr"]), 100 * left_out, worst))
        if len(c["corr"]) >= 48:
            assert left_out <= 0.25
    # ---- the two loop cases ----
    early = make_case(7, 257, 103, False, s=0.9, d=1.0 / 32)
    full = make_case(8, 48, 5, False, s=0.8, d=0.0)
    loops = dict(early=(early, 2048, 0.999), full=(full, 1000, 0.999))
    for name, (c, max_iteration, confidence) in loops.items():
        for k in ("P", "Q", "corr", "planted", "T_true", "params", "seed"):
            d[name + "/" + k] = c[k]
        d[name + "/ransac_n"] = np.array(c["ransac_n"])
        d[name + "/criteria"] = np.array([max_iteration, confidence])
        r, s, dd = c["params"]
        out = RR.ransac(c["P"], c["Q"], c["corr"], r, c["ransac_n"], max_iteration, confidence, int(c["seed"][0]), s, dd)
        print("%-5s trials %d of %d, valid %d, best trial %d, count %d of %d planted" % (
            name, out["trials"], max_iteration, out["valid_trials"], out["best_trial"], out["count"], c["planted"].sum()))
        if name == "early":
            assert 64 < out["trials"] < max_iteration and out["trials"] % 64 != 0
        else:
            assert out["trials"] == max_iteration and out["best_trial"] >= 0
        assert 0 < out["valid_trials"] < out["trials"]
    # the exact case: some trial inside the fixture's range draws three distinct planted pairs and recovers the pose
    c = cases["e255"]
    out = RR.ransac(c["P"], c["Q"], c["corr"], R_MATCH, 3, TRIALS, 0.999, int(c["seed"][0]))
    q = out["best_trial"]
    bar = 16.0 * max(float(d["e255/A"][q]), 2.0 ** -52 * float(d["e255/cond"][q]))
    assert out["count"] >= c["planted"].sum() and np.linalg.norm(out["transformation"] - c["T_true"]) <= bar
    assert np.abs(d["e255/gT"][q] - c["T_true"][:3].ravel()).max() < 1e-30  # the 50-digit pose IS the planted one
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
