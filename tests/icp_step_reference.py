"""One ICP step U of every estimation method (include/teaser_hip.h, "ICP refinement") on inputs whose arithmetic is
exact, computed at 50 digits.

Inputs.  Every coordinate, normal, covariance entry and displacement is a small dyadic rational, so every product and
sum of the contract's formulas -- the count, sum d2, the 15 point-to-point sums, the 21 + 6 entries of A and g -- is
representable in FP64 and comes out the same in ANY order of summation: the GPU's block, wave and tree order must give
exactly these sums, and an exactly singular system stays exactly singular on the device.  exact_sums() asserts this
for every case with fractions.Fraction: all terms of a sum are multiples of one power of two u and sum |term| < 2^53 u,
so no partial sum in any order can round.  (Robust-kernel weights other than 1 are rational, not dyadic: for those
cases the unweighted terms are asserted exact and the weights are carried as exact Fractions.)
Correspondences are forced: source points at least 1 apart, every target within r = 1/4 of exactly one source, so
with max_iteration = 1 the result's transformation is U init.

Reference.  The sums as exact Fractions; Umeyama through mpmath's svd_r at 50 digits; the 6 x 6 solve as the
contract's LDL^T in exact rational arithmetic with its pivot rule evaluated on the exact pivots, the rotation through
mpmath's sin / cos; Generalized ICP's M, adjugate, det and skip rule on exact values; kernel weights on exact
residuals.  Only the construction of the cases needs numpy alone; mpmath is imported when a step is computed."""
import functools
import math
from fractions import Fraction as Fr

import numpy as np

import icp_gicp_reference as RG
import icp_plane_reference as RP
import icp_reference as R

DIGITS = 50
POINT, PLANE, GICP = 0, 1, 2
R_MATCH = 0.25
COND_MAX = 1e3  # every case with a unique answer is at most this ill-conditioned, so no bar can hide a wrong branch


# ---- construction of the cases (numpy only) -------------------------------------------------------------------------
def lattice(nx, ny, nz, origin=(0, 0, 0)):
    """nx ny nz integer points, x fastest, shifted by origin."""
    i = np.arange(nx * ny * nz)
    return np.stack([i % nx, (i // nx) % ny, i // (nx * ny)], 1).astype(np.float64) + np.asarray(origin, np.float64)


def moved(P, w64=(0, 0, 0), t64=(0, 0, 0), seed=None, amp=1, unit=64.0):
    """q = p + w x p + t + delta with w, t and delta multiples of 1 / unit (delta: integers in [-amp, amp] per
    coordinate from the seed)."""
    w, t = np.asarray(w64, np.float64) / unit, np.asarray(t64, np.float64) / unit
    Q = P + np.cross(w, P) + t
    if seed is not None:
        Q = Q + np.random.default_rng(seed).integers(-amp, amp + 1, size=P.shape) / unit
    return Q


def signed_permutation(t64=(0, 0, 0)):
    """x -> (-y, z, -x) + t: a proper rotation whose entries are 0 and +-1."""
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [0, 0, 1], [-1, 0, 0]]
    T[:3, 3] = np.asarray(t64, np.float64) / 64
    return T


def preimage(X, init):
    """P with apply(init, P) = X for a signed permutation init (exact)."""
    return (X - init[:3, 3]) @ init[:3, :3]


def _case(name, method, P, Q, r=R_MATCH, init=None, N=None, Cs=None, Ct=None, kernel=0, k=1.0, kind="unique",
          store=True):
    return dict(name=name, method=method, P=np.ascontiguousarray(P, dtype=np.float64),
                Q=np.ascontiguousarray(Q, dtype=np.float64), r=float(r),
                init=np.eye(4) if init is None else np.asarray(init, np.float64), N=N, Cs=Cs, Ct=Ct, kernel=kernel,
                k=float(k), kind=kind, store=store)


def patch(n=8):
    """n x n points of the dyadic saddle z = (x^2 - y^2) / 4 over integer x, y and its unnormalised normals."""
    g = lattice(n, n, 1, (-n // 2, -n // 2, 0))
    x, y = g[:, 0], g[:, 1]
    S = np.stack([x, y, (x * x - y * y) / 4], 1)
    return S, np.stack([-x / 2, y / 2, np.ones_like(x)], 1)


def generic_normals(P):
    """Dyadic, unnormalised normals that vary with all three coordinates (multiples of 1/4)."""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([(np.mod(x + 2 * y + z, 5) - 2) / 4, (np.mod(y + 3 * z - x, 7) - 3) / 4,
                     1 + np.mod(x + z, 2) / 2], 1)


def axis_normals(P):
    """Integer normals cycling through nine axis and face-diagonal directions: a well-conditioned A on a cube."""
    D = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, -1, 0], [0, 1, -1], [-1, 0, 1]],
                 dtype=np.float64)
    return D[np.mod(P[:, 0] + 3 * P[:, 1] + 7 * P[:, 2], 9).astype(np.int64)]


def regular_covariances(X, init):
    """(Cs, Ct) with M = Ct + Rk Cs Rk^T one of a family of dyadic matrices of determinant 2^k, so W is dyadic: a 2 x 2
    block [[5/4, +-3/4], [+-3/4, 5/4]] (determinant 1) on a pair of axes and c in {1/2, 1, 2} on the third."""
    n = len(X)
    Rk = init[:3, :3]
    Cs, Ct = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    for i in range(n):
        a, b = [(0, 1), (0, 2), (1, 2)][i % 3]
        o = 3 - a - b
        M = np.zeros((3, 3))
        M[a, a] = M[b, b] = 1.25
        M[a, b] = M[b, a] = 0.75 if (i // 3) % 2 else -0.75
        M[o, o] = (0.5, 1.0, 2.0)[(i // 6) % 3]
        S = np.diag(np.roll([0.25, 0.125, 0.0625], i % 3))
        S[0, 1] = S[1, 0] = 0.03125 * ((i % 5) - 2)
        Cs[i] = S
        Ct[i] = M - Rk @ S @ Rk.T
    return Cs, Ct


def singular_covariances(n):
    """Cs = Ct = n n^T with n = e_z: M = n n^T + Rk n n^T Rk^T has rank <= 2, det(M) = 0 exactly."""
    C = np.zeros((n, 3, 3))
    C[:, 2, 2] = 1.0
    return C, C.copy()


def _method_case(name, method, X, Q, kind="unique", store=True, singular=None, r=R_MATCH, src_of=None):
    """A problem of `method` whose moved source is X: point-to-point and point-to-plane with the identity as init,
    Generalized ICP with the signed permutation (so B = Rk Cs Rk^T matters).  src_of[j]: the source target j was made
    from (default j); singular: a mask over the sources whose pair gets a singular M."""
    if method == POINT:
        return _case(name, POINT, X, Q, r, kind=kind, store=store)
    if method == PLANE:
        return _case(name, PLANE, X, Q, r, N=generic_normals(np.rint(Q)), kind=kind, store=store)
    init = signed_permutation((8, -16, 24))
    Cs, Ct = regular_covariances(X, init)
    if singular is not None:
        Cs[singular], Ct[singular] = singular_covariances(int(np.count_nonzero(singular)))
    if src_of is not None:
        Ct = Ct[src_of]
    return _case(name, GICP, preimage(X, init), Q, r, init=init, Cs=Cs, Ct=Ct, kind=kind, store=store)


def _single_pair(name, method, n_s, at, store=True):
    """n_s sources of which only source `at` has a target.  Point-to-point: H = 0, R = I.  The other two methods: an
    exactly singular A whose LDL^T meets an exactly zero pivot in FP64 too (the divisors are powers of two)."""
    X = lattice(16, 16, max(1, (n_s + 255) // 256), (-8, -8, 0))[:n_s]
    far = np.array([[100.0, 100.0, 100.0]])
    if method == POINT:
        Q = np.concatenate([far, X[at:at + 1] + [0.125, -0.0625, 0.03125]])
        return _case(name, POINT, X, Q, kind="maximiser", store=store)
    if method == PLANE:
        Q = X[at:at + 1] - [0.125, 0.125, 0.125]
        return _case(name, PLANE, X, Q, N=np.array([[0.0, 0.0, 1.0]]), kind="identity", store=store)
    Q = X[at:at + 1] - [0.0, 0.0, 0.125]
    C = np.tile(np.eye(3) / 4, (n_s, 1, 1))
    return _case(name, GICP, X, Q, Cs=C, Ct=C[:1].copy(), kind="identity", store=store)


def point_cases():
    out = []
    X = lattice(2, 2, 1)
    out.append(_case("pt_1", POINT, X, np.array([[1.125, -0.0625, 0.03125], [9.0, 9.0, 9.0]]), kind="maximiser"))
    out.append(_case("pt_2", POINT, X, moved(X[[3, 0]], (1, -2, 3), (4, 2, -3)), kind="maximiser"))
    tri = np.array([[0.0, 0, 0], [3, 0, 0], [0, 2, 0], [7, 7, 7]])
    out.append(_case("pt_3_triangle", POINT, tri, moved(tri[:3], (2, -1, 3), (3, -2, 5))))
    quad = lattice(2, 2, 1) * [2.0, 1.0, 1.0]
    out.append(_case("pt_4_coplanar", POINT, quad, moved(quad, (3, -2, 2), (-3, 4, 6), seed=4)))
    line = lattice(5, 1, 1, (-2, 0, 0))
    out.append(_case("pt_5_collinear", POINT, line, moved(line, (2, 3, -4), (5, -2, 3)), kind="maximiser"))
    cube = lattice(4, 4, 4, (-2, -2, -2))
    out.append(_case("pt_64", POINT, cube, moved(cube, (1, -1, 2), (2, -1, 1), seed=64)))
    # a thin slab (integer x, y; |z| <= 1/16) whose target is its mirror image in z, shifted: det(H) < 0, s1 > s2 > 0
    slab = lattice(6, 4, 1)
    slab[:, 2] = np.array([2, -2, 1, -1, -2, 2, -1, 1])[(np.arange(24) * 5) % 8] / 32
    out.append(_case("pt_mirror_slab", POINT, slab, slab * [1.0, 1.0, -1.0] + np.array([2, -1, 0]) / 64))
    octa = np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    out.append(_case("pt_isotropic", POINT, octa, octa + np.array([4, -2, 6]) / 64))
    out.append(_case("pt_all_to_one", POINT, lattice(3, 3, 1), np.array([[1.0, 1.0, 0.125]]), r=4.0, kind="maximiser"))
    return out


def _edge_patch(name, kernel, k):
    """The patch with the source displaced along z alone (n_z = 1, so the residual IS the displacement): residuals
    exactly +-k, one step of 1/64 either side of it, 2 k, and smaller ones."""
    S, N = patch()
    steps = np.array([0, 64 * k, -64 * k, 64 * k + 1, -(64 * k + 1), 64 * k - 1, -(64 * k - 1), 128 * k, 1, -2, 3])
    X = S.copy()
    X[:, 2] += steps[(np.arange(len(S)) * 7) % len(steps)] / 64
    return _case(name, PLANE, X, S, N=N, kernel=kernel, k=k)


def plane_cases():
    out = []
    flat = lattice(6, 5, 1, (-3, -2, 0))
    Qf = moved(flat, (2, -1, 1), (3, -2, 4), seed=7)
    Qf[:, 2] = 0.125  # a planar target
    out.append(_case("pl_parallel_normals", PLANE, flat, Qf, N=np.tile([0.0, 0.0, 1.5], (30, 1)), kind="identity"))
    out.append(_case("pl_zero_normals", PLANE, flat, Qf, N=np.zeros((30, 3)), kind="identity"))
    out.append(_single_pair("pl_one", PLANE, 4, 2))
    S, N = patch()
    Qp = moved(S, (1, -1, 1), (2, -1, 3), seed=11)
    out.append(_case("pl_patch", PLANE, S, Qp, N=N))
    # e = x - q perpendicular to n in every pair: e = (a, b, (a x - b y) / 2) with a = b = 1/32; g = 0, xi = 0, U = I
    e = np.stack([np.full(64, 1 / 32), np.full(64, 1 / 32), (S[:, 0] - S[:, 1]) / 64], 1)
    out.append(_case("pl_zero_residuals", PLANE, S + e, S, N=N))
    out.append(_edge_patch("pl_huber_edge", 1, 1 / 16))
    out.append(_edge_patch("pl_tukey_edge", 4, 1 / 16))
    out.append(_case("pl_cauchy", PLANE, S, Qp, N=N, kernel=2, k=1 / 8))
    out.append(_case("pl_gm", PLANE, S, Qp, N=N, kernel=3, k=1 / 8))
    return out


def gicp_cases():
    X = lattice(4, 4, 4, (-2, -2, -2))
    Q = moved(X, (1, -1, 2), (2, -1, 1), seed=64)
    every_third = np.arange(64) % 3 == 1
    return [_method_case("gi_regular", GICP, X, Q),
            _method_case("gi_mixed_singular", GICP, X, Q, singular=every_third),
            _method_case("gi_all_singular", GICP, X, Q, kind="identity", singular=np.ones(64, bool))]


BIG_N = 65793  # 257 blocks of 256: the finalize loop's second trip


def granularity_cases():
    out = []
    for method, tag in ((POINT, "pt"), (PLANE, "pl"), (GICP, "gi")):
        out.append(_single_pair("g%s_1" % tag, method, 1, 0))
        for n in (255, 256, 257, 513):
            X = lattice(8, 8, 9, (-4, -4, -4))[:n]
            out.append(_method_case("g%s_%d" % (tag, n), method, X, moved(X, (1, -1, 1), (2, -3, 1), seed=n)))
        X = lattice(16, 16, 3, (-8, -8, -1))
        keep = np.r_[0:256, 512:768]  # the middle block of 256 has no match at all
        out.append(_method_case("g%s_768_gap" % tag, method, X, moved(X[keep], (0, 0, 1), (2, -3, 1), seed=768),
                                src_of=keep))
        out.append(_single_pair("g%s_512_last" % tag, method, 512, 511))
    return out


def big_case(method):
    """65 793 sources, every one matched; coordinates are integers, the motion a translation plus noise, both in
    sixteenths."""
    X = lattice(41, 41, 40, (-20, -20, -20))[:BIG_N]
    Q = moved(X, (0, 0, 0), (1, -1, 1), seed=65793, amp=1, unit=16.0)
    if method == POINT:
        return _case("gpt_65793", POINT, X, Q, store=False)
    return _case("gpl_65793", PLANE, X, Q, N=axis_normals(X), store=False)


def near_singular_cases():
    """Planar inputs with roughness of the order 2^-30: legitimately ill-conditioned, no expected answer."""
    flat = lattice(6, 5, 1, (-3, -2, 0))
    rough = (np.mod(np.arange(30) * 7, 11) - 5) * 2.0 ** -30
    Xr = flat.copy()
    Xr[:, 2] = rough
    Qm = moved(flat, (0, 0, 1), (3, -2, 4), seed=7)
    Qm[:, 2] = -rough + 0.125
    N = np.stack([rough, -rough[::-1], np.ones(30)], 1)
    C = np.zeros((30, 3, 3))
    C[:, 2, 2] = 1.0
    C += np.eye(3) * 2.0 ** -30
    return [_case("near_pt", POINT, Xr, Qm, kind="near", store=False),
            _case("near_pl", PLANE, flat, Qm, N=N, kind="near", store=False),
            _case("near_gi", GICP, flat, Qm, Cs=C, Ct=C.copy(), kind="near", store=False)]


def small_cases():
    return point_cases() + plane_cases() + gicp_cases() + granularity_cases()


def all_reference_cases():
    return small_cases() + [big_case(POINT), big_case(PLANE)]


# ---- exact correspondences ------------------------------------------------------------------------------------------
def _ints(a, unit):
    s = np.asarray(a, np.float64) * unit
    assert np.array_equal(s, np.rint(s)) and np.abs(s).max(initial=0) < 2.0 ** 30, "not a multiple of 1/%d" % unit
    return s.astype(np.int64)


def match(c, X):
    """The contract's corr on exact integers (units of 2^-12): per source the lexicographic minimum of (d2, j) over the
    targets with d2 < r r, or -1; also d2 in units of 2^-24.  Asserts that the sources are at least 1 apart and that
    every matched target is within r of exactly one source."""
    Xi, Qi = _ints(X, 4096), _ints(c["Q"], 4096)
    r2 = _ints(c["r"] * c["r"], 4096 * 4096)
    one = 4096 * 4096
    n_s, n_t = len(Xi), len(Qi)
    if n_s * n_t <= 4_000_000:
        d2 = ((Xi[:, None, :] - Qi[None, :, :]) ** 2).sum(-1)
        inside = d2 < r2
        big = np.iinfo(np.int64).max
        j = np.where(inside.any(1), np.argmin(np.where(inside, d2, big), 1), -1)  # argmin: the first on a tie
        if c["r"] <= R_MATCH:
            assert (inside.sum(0) <= 1).all(), "a target within r of two sources"
            gram = ((Xi[:, None, :] - Xi[None, :, :]) ** 2).sum(-1) + np.eye(n_s, dtype=np.int64) * one
            assert gram.min() >= one, "sources closer than 1"
    else:  # integer sources, r <= 1/4: a target within r of a source rounds to it
        assert c["r"] <= R_MATCH and np.array_equal(Xi % 4096, np.zeros_like(Xi))
        key = lambda a: ((a[:, 0] + 2048) * 4096 + (a[:, 1] + 2048)) * 4096 + (a[:, 2] + 2048)
        ks = key(Xi // 4096)
        order = np.argsort(ks, kind="stable")
        assert (np.diff(ks[order]) > 0).all(), "sources not distinct"
        kq = key(np.rint(c["Q"]).astype(np.int64))
        pos = np.clip(np.searchsorted(ks[order], kq), 0, n_s - 1)
        src = order[pos]
        d2t = ((Xi[src] - Qi) ** 2).sum(-1)
        ok = (ks[src] == kq) & (d2t < r2)
        j = np.full(n_s, -1, dtype=np.int64)
        for t in np.lexsort((-np.arange(n_t), -d2t))[::1]:  # descending (d2, j): the minimum is written last
            if ok[t]:
                j[src[t]] = t
    m = j >= 0
    d2m = ((Xi[m] - Qi[j[m]]) ** 2).sum(-1)
    return j, d2m


# ---- exact sums -------------------------------------------------------------------------------------------------------
def _fits(terms, den, summed=True):
    """True when every term (value = term / den, term an integer or a Fraction) is a multiple of one power of two u and
    sum |term| < 2^53 u (summed) or max |term| < 2^53 u: then no partial sum in any order rounds in FP64."""
    flat = [Fr(t) for t in (terms.ravel() if isinstance(terms, np.ndarray) else terms)]
    d = functools.reduce(lambda a, b: a * b // math.gcd(a, b), [f.denominator for f in flat], 1) * den
    if d & (d - 1):
        return False
    nums = [abs(int(f * d // den)) for f in flat]
    tot = sum(nums) if summed else max(nums, default=0)
    if tot == 0:
        return True
    g = functools.reduce(math.gcd, nums, d)
    return tot // (g & -g) < 2 ** 53


def _obj(a, scale):
    a = np.asarray(a, np.float64)
    if scale is None:
        vals = [Fr(float(v)) for v in a.ravel()]
    else:
        s = a * scale
        assert np.array_equal(s, np.rint(s)) and np.abs(s).max(initial=0) < 2.0 ** 52
        vals = [int(v) for v in s.ravel()]
    out = np.empty(a.size, dtype=object)
    out[:] = vals
    return out.reshape(a.shape)


def _scale_for(c):
    """The smallest power of two that makes every input of the case, and the target's bounding-box centre, an
    integer."""
    arrs = [c["P"], c["Q"], c["init"][:3, 3], RP.centre_of(c["Q"])] + ([c["N"]] if c["N"] is not None else [])
    for e in range(0, 40):
        if all(np.array_equal(a * 2.0 ** e, np.rint(a * 2.0 ** e)) for a in arrs):
            return 2 ** e
    raise AssertionError("inputs are not small dyadic rationals")


def weight_exact(kernel, k, r):
    """Open3D's RobustKernel::Weight on an exact residual: a Fraction (every kernel's weight is rational in r, k)."""
    k, a = Fr(float(k)), abs(r)
    if kernel == 0:
        return Fr(1)
    if kernel == 1:
        return Fr(1) if a <= k else k / a
    if kernel == 2:
        return 1 / (1 + (r / k) ** 2)
    if kernel == 3:
        return k / (k + r * r) ** 2
    if kernel == 4:
        return (1 - (r / k) ** 2) ** 2 if a <= k else Fr(0)
    raise ValueError(kernel)


def exact_sums(c, mode=None):
    """The sums of the case's one correspondence pass as exact Fractions, with the assertion that FP64 holds them and
    every intermediate exactly.  mode 'int' computes on scaled Python integers (fast; L2 point-to-point and
    point-to-plane), 'fraction' on Fractions; the default picks 'int' where it applies.
    Returns dict(j, cnt, d2, centre, X (float64, moved by init), exact (bool: the weighted sums are exact too) and per
    method sp, sq, spq | A, g)."""
    method, kernel = c["method"], c["kernel"]
    if mode is None:
        mode = "int" if method != GICP and kernel == 0 else "fraction"
    assert mode == "fraction" or (method != GICP and kernel == 0)
    scale = _scale_for(c) if mode == "int" else None
    unit = Fr(1, scale) if scale else Fr(1)
    den = (lambda deg: scale ** deg) if scale else (lambda deg: 1)
    init = c["init"]
    Rk = [[int(v) for v in row] for row in init[:3, :3]]
    assert np.array_equal(init[:3, :3], np.array(Rk, dtype=np.float64)) and np.array_equal(init[3], [0, 0, 0, 1])
    assert all(sorted(abs(v) for v in row) == [0, 0, 1] for row in Rk), "init's rotation is no signed permutation"
    Po, to = _obj(c["P"], scale), _obj(init[:3, 3], scale)
    Xo = np.empty_like(Po)
    for r in range(3):
        Xo[:, r] = Rk[r][0] * Po[:, 0] + Rk[r][1] * Po[:, 1] + Rk[r][2] * Po[:, 2] + to[r]
    X = R.apply(init, c["P"])  # the device's expression; exact, hence equal to Xo
    assert np.array_equal(_obj(X, scale), Xo)
    j, d2m = match(c, X)
    m = j >= 0
    cnt = int(m.sum())
    Qo = _obj(c["Q"], scale)
    lo, hi = Qo.min(0), Qo.max(0)
    co = (lo + hi) / 2 if scale is None else (lo + hi) // 2
    assert np.array_equal(_obj(RP.centre_of(c["Q"]), scale), co), "the bounding-box centre is not representable"
    out = dict(j=j, cnt=cnt, X=X, centre=[Fr(v) * unit for v in co], d2=Fr(int(d2m.sum()), 4096 * 4096))
    assert int(d2m.sum()) < 2 ** 53
    xp, qp = Xo[m] - co, Qo[j[m]] - co
    e = xp - qp
    ok = _fits(xp, den(1), False) and _fits(qp, den(1), False) and _fits(e, den(1), False)
    exact = True
    if method == POINT:
        sp, sq = xp.sum(0) if cnt else np.zeros(3, object), qp.sum(0) if cnt else np.zeros(3, object)
        spq = np.zeros((3, 3), dtype=object)
        for r in range(3):
            ok = ok and _fits(xp[:, r], den(1)) and _fits(qp[:, r], den(1))
            for q in range(3):
                t = xp[:, r] * qp[:, q]
                ok = ok and _fits(t, den(2))
                spq[r, q] = t.sum() if cnt else 0
        out.update(sp=[Fr(v) * unit for v in sp], sq=[Fr(v) * unit for v in sq],
                   spq=[[Fr(v) * unit ** 2 for v in row] for row in spq])
    elif method == PLANE:
        No = _obj(c["N"], scale)[j[m]]
        res = e[:, 0] * No[:, 0] + e[:, 1] * No[:, 1] + e[:, 2] * No[:, 2]
        J = [xp[:, 1] * No[:, 2] - xp[:, 2] * No[:, 1], xp[:, 2] * No[:, 0] - xp[:, 0] * No[:, 2],
             xp[:, 0] * No[:, 1] - xp[:, 1] * No[:, 0], No[:, 0], No[:, 1], No[:, 2]]
        dj = [2, 2, 2, 1, 1, 1]
        ok = ok and _fits(res, den(2), False) and all(_fits(J[r], den(dj[r]), False) for r in range(6))
        if kernel == 0:
            w = None
        else:
            w = np.empty(cnt, dtype=object)
            w[:] = [weight_exact(kernel, c["k"], v) for v in res]
        A = [[Fr(0)] * 6 for _ in range(6)]
        g = [Fr(0)] * 6
        for r in range(6):
            wj = J[r] if w is None else w * J[r]
            for q in range(r, 6):
                t = wj * J[q]
                ok = ok and _fits(J[r] * J[q], den(dj[r] + dj[q]))
                exact = exact and (w is None or _fits(t, 1))
                A[r][q] = A[q][r] = Fr(t.sum() if cnt else 0) * unit ** (dj[r] + dj[q])
            t = (res if w is None else w * res) * J[r]
            ok = ok and _fits(res * J[r], den(2 + dj[r]))
            exact = exact and (w is None or _fits(t, 1))
            g[r] = Fr(t.sum() if cnt else 0) * unit ** (2 + dj[r])
        out.update(A=A, g=g, residuals=[Fr(v) * unit ** 2 for v in res])
    else:
        A, g, skipped = _gicp_sums(c, Rk, xp, e, j, m)
        ok = ok and A is not None
        out.update(A=A, g=g, skipped=skipped)
    assert ok, "%s: a sum or an intermediate is not exact in FP64" % c["name"]
    out["exact"] = bool(exact)
    return out


def _gicp_sums(c, Rk, xp, e, j, m):
    """(A, g, number of pairs left out) as Fractions; A is None when some term is not exact in FP64."""
    Cs, Ct = RG.sym_upper(c["Cs"])[m], RG.sym_upper(c["Ct"])[j[m]]
    A = [[Fr(0)] * 6 for _ in range(6)]
    g = [Fr(0)] * 6
    terms = [[[] for _ in range(6)] for _ in range(7)]
    inter = []  # M, W and det of every contributing pair
    skipped = 0
    for i in range(len(xp)):
        s = [Fr(float(v)) for v in Cs[i]]
        S = [[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]]
        B = [[sum(Rk[r][k] * S[k][q] for k in range(3)) for q in range(3)] for r in range(3)]
        t = [Fr(float(v)) for v in Ct[i]]
        T = [[t[0], t[1], t[2]], [t[1], t[3], t[4]], [t[2], t[4], t[5]]]
        M = [[T[r][q] + sum(B[r][k] * Rk[q][k] for k in range(3)) for q in range(3)] for r in range(3)]
        a00, a01 = M[1][1] * M[2][2] - M[1][2] * M[1][2], M[0][2] * M[1][2] - M[0][1] * M[2][2]
        a02, a11 = M[0][1] * M[1][2] - M[0][2] * M[1][1], M[0][0] * M[2][2] - M[0][2] * M[0][2]
        a12, a22 = M[0][1] * M[0][2] - M[0][0] * M[1][2], M[0][0] * M[1][1] - M[0][1] * M[0][1]
        det = M[0][0] * a00 + M[0][1] * a01 + M[0][2] * a02
        if not det > 0:
            skipped += 1
            continue
        W = [[a00 / det, a01 / det, a02 / det], [a01 / det, a11 / det, a12 / det], [a02 / det, a12 / det, a22 / det]]
        x, ee = list(xp[i]), list(e[i])
        we = [sum(W[r][k] * ee[k] for k in range(3)) for r in range(3)]
        G = [[x[1] * W[2][k] - x[2] * W[1][k] for k in range(3)], [x[2] * W[0][k] - x[0] * W[2][k] for k in range(3)],
             [x[0] * W[1][k] - x[1] * W[0][k] for k in range(3)]]
        Ai = [[Fr(0)] * 6 for _ in range(6)]
        for r in range(3):
            Ai[r][0] = x[1] * G[r][2] - x[2] * G[r][1]
            Ai[r][1] = x[2] * G[r][0] - x[0] * G[r][2]
            Ai[r][2] = x[0] * G[r][1] - x[1] * G[r][0]
            for k in range(3):
                Ai[r][3 + k] = G[r][k]
                Ai[3 + r][3 + k] = W[r][k]
        gi = [x[1] * we[2] - x[2] * we[1], x[2] * we[0] - x[0] * we[2], x[0] * we[1] - x[1] * we[0]] + we
        for r in range(6):
            for q in range(r, 6):
                terms[r][q].append(Ai[r][q])
                A[r][q] += Ai[r][q]
            terms[6][r].append(gi[r])
            g[r] += gi[r]
        inter += [v for row in M for v in row] + [v for row in W for v in row] + [det]
    for r in range(6):
        for q in range(r + 1, 6):
            A[q][r] = A[r][q]
    fine = all(_fits(t, 1) for row in terms for t in row if t) and _fits(inter, 1, False)
    return (A if fine else None), g, skipped


# ---- the step at 50 digits ------------------------------------------------------------------------------------------
def context():
    import mpmath
    ctx = mpmath.MPContext()
    ctx.dps = DIGITS
    return ctx


def _mpf(ctx, f):
    f = Fr(f)
    return ctx.mpf(f.numerator) / f.denominator


def _rank(H):
    M = [row[:] for row in H]
    rank = 0
    for col in range(3):
        piv = next((r for r in range(rank, 3) if M[r][col] != 0), None)
        if piv is None:
            continue
        M[rank], M[piv] = M[piv], M[rank]
        for r in range(rank + 1, 3):
            f = M[r][col] / M[rank][col]
            M[r] = [a - f * b for a, b in zip(M[r], M[rank])]
        rank += 1
    return rank


def umeyama_step(ctx, s):
    """dict(U (4 x 4 mp matrix, or None when R is not unique), sv (the singular values, exact zeros where the exact
    rank says so), d, rank, unique, cond, H, mu_p, mu_q) from the exact sums."""
    n = s["cnt"]
    H = [[s["spq"][r][q] - s["sp"][r] * s["sq"][q] / n for q in range(3)] for r in range(3)]
    rank = _rank(H)
    det = (H[0][0] * (H[1][1] * H[2][2] - H[1][2] * H[2][1]) - H[0][1] * (H[1][0] * H[2][2] - H[1][2] * H[2][0]) +
           H[0][2] * (H[1][0] * H[2][1] - H[1][1] * H[2][0]))
    d = -1 if det < 0 else 1
    mu_p = [s["centre"][r] + s["sp"][r] / n for r in range(3)]
    mu_q = [s["centre"][r] + s["sq"][r] / n for r in range(3)]
    out = dict(rank=rank, d=d, H=H, mu_p=mu_p, mu_q=mu_q, U=None, unique=False, cond=float("inf"))
    if rank == 0:
        out["sv"] = [ctx.mpf(0)] * 3
        return out
    Hm = ctx.matrix([[_mpf(ctx, v) for v in row] for row in H])
    U, S, Vt = ctx.svd_r(Hm)
    order = sorted(range(3), key=lambda k: -S[k])
    sv = [S[k] if pos < rank else ctx.mpf(0) for pos, k in enumerate(order)]
    out["sv"] = sv
    tie = d < 0 and abs(sv[1] - sv[2]) <= ctx.mpf(10) ** -40 * sv[0]
    out["unique"] = rank >= 2 and not tie
    if not out["unique"]:
        return out
    out["cond"] = float(sv[0] / (sv[1] + d * sv[2]))
    Uo = ctx.matrix(3, 3)
    Vo = ctx.matrix(3, 3)
    for pos, k in enumerate(order):
        for r in range(3):
            Uo[r, pos] = U[r, k]
            Vo[r, pos] = Vt[k, r]
    D = ctx.eye(3)
    D[2, 2] = -1 if ctx.det(Uo) * ctx.det(Vo) < 0 else 1
    Rm = Vo * D * Uo.T
    mp_p = ctx.matrix([_mpf(ctx, v) for v in mu_p])
    mp_q = ctx.matrix([_mpf(ctx, v) for v in mu_q])
    t = mp_q - Rm * mp_p
    T = ctx.eye(4)
    for r in range(3):
        for q in range(3):
            T[r, q] = Rm[r, q]
        T[r, 3] = t[r]
    out["U"] = T
    return out


def ldl_solve(A, g):
    """The contract's LDL^T without pivoting on exact values: xi as Fractions, or None when a pivot is not > 0."""
    L = [[Fr(0)] * 6 for _ in range(6)]
    d = [Fr(0)] * 6
    for j in range(6):
        s = A[j][j] - sum(L[j][k] * L[j][k] * d[k] for k in range(j))
        if not s > 0:
            return None
        d[j] = s
        for i in range(j + 1, 6):
            L[i][j] = (A[i][j] - sum(L[i][k] * L[j][k] * d[k] for k in range(j))) / s
    y = [Fr(0)] * 6
    for i in range(6):
        y[i] = -g[i] - sum(L[i][k] * y[k] for k in range(i))
    y = [y[i] / d[i] for i in range(6)]
    xi = [Fr(0)] * 6
    for i in range(5, -1, -1):
        xi[i] = y[i] - sum(L[k][i] * xi[k] for k in range(i + 1, 6))
    return xi


def six_step(ctx, s):
    """dict(U (4 x 4 mp matrix; the identity when the exact LDL^T meets a pivot that is not positive), identity, cond
    (of A, inf when singular)) from the exact A, g and centre."""
    xi = ldl_solve(s["A"], s["g"]) if s["cnt"] else None
    if xi is None:
        return dict(U=ctx.eye(4), identity=True, cond=float("inf"))
    sv = ctx.svd_r(ctx.matrix([[_mpf(ctx, v) for v in row] for row in s["A"]]), compute_uv=False)
    x = [_mpf(ctx, v) for v in xi]
    c = [_mpf(ctx, v) for v in s["centre"]]
    ca, sa, cb, sb, cg, sg = ctx.cos(x[0]), ctx.sin(x[0]), ctx.cos(x[1]), ctx.sin(x[1]), ctx.cos(x[2]), ctx.sin(x[2])
    Rm = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
          [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa], [-sb, cb * sa, cb * ca]]
    U = ctx.eye(4)
    for r in range(3):
        for q in range(3):
            U[r, q] = Rm[r][q]
        U[r, 3] = x[3 + r] + c[r] - (Rm[r][0] * c[0] + Rm[r][1] * c[1] + Rm[r][2] * c[2])
    return dict(U=U, identity=False, cond=float(max(sv) / min(sv)))


def restatement(c, s):
    """U of the project's FP64 restatements (icp_reference.umeyama, icp_plane_reference.plane_step, the Generalized-ICP
    restatement's gicp_step) on the case's correspondences."""
    j, X = s["j"], s["X"]
    m = j >= 0
    Q = c["Q"][j[m]]
    centre = RP.centre_of(c["Q"])
    if c["method"] == POINT:
        return R.umeyama(X[m], Q)
    if c["method"] == PLANE:
        return RP.plane_step(X[m], Q, c["N"][j[m]], centre, RP.KERNELS[c["kernel"]], c["k"])
    return RG.gicp_step(X[m], Q, RG.sym_upper(c["Cs"])[m], RG.sym_upper(c["Ct"])[j[m]], c["init"][:3, :3], centre)


def float_sums(s):
    """(A, g) of a 6 x 6 case as float64 arrays (exact when s['exact'])."""
    return (np.array([[float(v) for v in row] for row in s["A"]]), np.array([float(v) for v in s["g"]]))


def reference(c, ctx=None):
    """Everything the fixture records for one case: T = U init rounded to FP64 (NaN where R is not unique), the
    case's condition, singular values, H, means, count, fitness and RMSE of the pass, the error of the FP64
    restatement against the 50-digit step, and whether the pass after the step keeps the correspondences."""
    ctx = ctx or context()
    s = exact_sums(c)
    n_s, cnt = len(c["P"]), s["cnt"]
    rec = dict(cnt=np.int64(cnt), fitness=np.float64(cnt / n_s if cnt else 0.0),
               rmse=np.float64(float(ctx.sqrt(_mpf(ctx, s["d2"]) / cnt)) if cnt else 0.0),
               match=s["j"].astype(np.int32), exact=np.bool_(s["exact"]), skipped=np.int64(s.get("skipped", 0)),
               sv=np.full(3, np.nan), H=np.full((3, 3), np.nan), mu_p=np.full(3, np.nan), mu_q=np.full(3, np.nan),
               d=np.int64(0), rank=np.int64(-1))
    if c["method"] == POINT:
        st = umeyama_step(ctx, s)
        unique = st["unique"]
        rec.update(sv=np.array([float(v) for v in st["sv"]]), d=np.int64(st["d"]), rank=np.int64(st["rank"]),
                   H=np.array([[float(v) for v in row] for row in st["H"]]),
                   mu_p=np.array([float(v) for v in st["mu_p"]]), mu_q=np.array([float(v) for v in st["mu_q"]]))
        assert unique == (c["kind"] == "unique"), (c["name"], st["rank"], st["d"])
    else:
        st = six_step(ctx, s)
        unique = not st["identity"]
        assert st["identity"] == (c["kind"] == "identity"), c["name"]
        A, g = float_sums(s)
        if st["identity"] and s["exact"]:  # the device's own arithmetic meets the zero pivot too
            assert cnt == 0 or RP.solve6(A, g) is None, c["name"]
    rec["cond"] = np.float64(st["cond"])
    init = ctx.matrix(c["init"].tolist())
    if unique or c["method"] != POINT:
        Tm = st["U"] * init
        rec["T"] = np.array([[float(Tm[r, q]) for q in range(4)] for r in range(4)])
    else:
        Tm = None
        rec["T"] = np.full((4, 4), np.nan)
    rec["err_fp64"] = np.float64(np.nan)
    if unique:
        assert st["cond"] <= COND_MAX, (c["name"], st["cond"])
        Tr = R.compose(restatement(c, s), c["init"])
        rec["err_fp64"] = np.float64(float(ctx.sqrt(sum((ctx.mpf(float(Tr[r, q])) - Tm[r, q]) ** 2
                                                        for r in range(4) for q in range(4)))))
    # does the pass after the step see the same correspondences?  Sources stay 1 apart and every target was within 1/4
    # of its own source, so a foreign target stays further than 1 - 1/4 - step > 1/4 from a source that moves by
    # step < 0.45; the pairs themselves must end within 0.9 r.
    keeps = False
    if Tm is not None and c["r"] <= R_MATCH:
        U = rec["T"] @ np.linalg.inv(c["init"])
        Xn = R.apply(U, s["X"])
        m = s["j"] >= 0
        step = np.linalg.norm(Xn - s["X"], axis=1).max(initial=0.0)
        gap = np.linalg.norm(Xn[m] - c["Q"][s["j"][m]], axis=1).max(initial=0.0)
        keeps = bool(step < 0.45 and gap < 0.9 * c["r"])
    rec["keeps"] = np.bool_(keeps)
    return rec
