"""CPU model of one axis of the fast route's translation in estimate_fused_kernel (csrc/kernels_estimate.hip), for
tests/test_fused_translation_model.py: the scalar TLS of registration.cc:21-88 with all ranges equal (beta), in its WINDOW
form.  The kernel's steps, in its order and with its association of every sum (the library is built without FMA
contraction, so numpy's separately rounded operations are the device's):

  sort        the K values ascending (the kernel pads its 512 slots with +inf, which sort behind every value)
  prefix      exclusive prefix sums p1 of x and p2 of x^2 over the sorted order -- lane-local sums of 8 values, a
              Hillis-Steele scan over the 64 lanes, then the lane's running sum
  endpoints   value i opens at x_i - beta and closes at x_i + beta.  After its opening the consensus set is the window
              [lo, i + 1) with lo = #{ j : x_j + beta < x_i - beta } (closings strictly before the opening); after its
              closing it is [i + 1, hi) with hi = #{ j : x_j - beta <= x_i + beta } (an opening of equal value goes
              first).  Both counts by binary search over the sorted values
  pos         the endpoint's rank in the merged order: i + lo for the opening, i + hi for the closing
  cost        window sums from the prefix sums, x_hat = s1 / card, residual = card x_hat^2 + s2 - 2 s1 x_hat,
              cost = residual + beta (K - card).  A window of ONE value is evaluated exactly: x_hat = the value,
              residual = 0 -- what the reference's sweep yields when consensus sets do not overlap (its running sums
              return to exactly 0 in between).  `exact_singletons=False` gives the rule before that: the prefix
              difference (a + b) - a, which is not b in general
  minimum     smallest cost, ties to the smaller pos; NaN (an empty window) never wins; if no cost is finite, the first
              endpoint's x_hat
"""
import numpy as np

LANES, E = 64, 8   # kFuseE values per lane, kFuseMaxK = LANES * E
MAX_K = LANES * E


def prefix_sums(sx, K):
    """p1, p2 [K + 1] as the kernel forms them (sx: the K sorted values)"""
    v = np.zeros(MAX_K)
    v[:K] = sx
    live = (np.arange(MAX_K) < K).reshape(LANES, E)
    v = v.reshape(LANES, E)
    out = []
    for w in (v, v * v):
        l = np.zeros(LANES)
        for r in range(E):   # lane-local, in register order
            l = np.where(live[:, r], l + w[:, r], l)
        inc = l.copy()
        o = 1
        while o < LANES:     # __shfl_up scan
            t = np.concatenate([np.zeros(o), inc[:-o]])
            inc = np.where(np.arange(LANES) >= o, inc + t, inc)
            o <<= 1
        e = inc - l          # exclusive
        p = np.zeros(MAX_K + 1)
        for r in range(E):
            p[np.arange(LANES) * E + r] = e
            e = np.where(live[:, r], e + w[:, r], e)
        p[MAX_K] = e[LANES - 1]   # the K == 512 line of the kernel
        out.append(p[:K + 1].copy())
    return out


def _count(pred, K):
    """the kernel's binary search: number of leading j with pred(j) true (pred is monotone over the sorted values)"""
    lo, n = 0, K
    while n > 0:
        half = n >> 1
        if pred(lo + half):
            lo += half + 1
            n -= half + 1
        else:
            n = half
    return lo


def fused_tls(x, beta, exact_singletons=True, detail=False, opening_first=True):
    """estimate of one axis; detail=True: (estimate, cost, pos, candidates [(pos, lo, hi, cost, x_hat)]).
    opening_first=False: the closing search with < instead of <= -- NOT the other tie order but a broken one (the window
    (x_i, x_i + 2 beta] after a closing loses its tied members and is evaluated nowhere else); kept to show that
    TIE_CASES of tests/estimator_cases.py tell the two apart."""
    x = np.asarray(x, dtype=np.float64)
    K = x.size
    assert 2 <= K <= MAX_K
    beta = np.float64(beta)
    sx = np.sort(x)
    p1, p2 = prefix_sums(sx, K)
    best = (np.inf, np.nan, 0x7fffffff)
    cands = []

    def consider(lo, hi, pos):
        nonlocal best
        with np.errstate(invalid="ignore", divide="ignore"):
            card = np.float64(hi - lo)
            if exact_singletons and hi - lo == 1:
                x_hat, residual = sx[lo], np.float64(0.0)
            else:
                s1, s2 = p1[hi] - p1[lo], p2[hi] - p2[lo]
                x_hat = s1 / card
                residual = card * x_hat * x_hat + s2 - 2 * s1 * x_hat
            c = residual + beta * np.float64(K - (hi - lo))
        cands.append((pos, lo, hi, float(c), float(x_hat)))
        if c < best[0] or (c == best[0] and pos < best[2]):
            best = (c, x_hat, pos)

    for i in range(K):
        av, bv = sx[i] - beta, sx[i] + beta
        lo = _count(lambda j: sx[j] + beta < av, K)
        consider(lo, i + 1, i + lo)
        hi = _count((lambda j: sx[j] - beta <= bv) if opening_first else (lambda j: sx[j] - beta < bv), K)
        consider(i + 1, hi, i + hi)
    est = best[1]
    if not best[0] < np.inf:
        est = p1[1] - p1[0]
    if detail:
        return float(est), float(best[0]), best[2], sorted(cands)
    return float(est)


def inliers(x, est, beta):
    return np.abs(np.asarray(x, dtype=np.float64) - est) <= beta
