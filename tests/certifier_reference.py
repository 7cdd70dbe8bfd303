"""Reference side of the certifier's stage tests (tests/test_gpu_certifier_stages.py, tests/test_certifier_reference.py)
-- TEST INFRASTRUCTURE ONLY.

  * dense_minit: M_init = Q_bar - mu J - lambda_guess, dense, from oracle/certifier.py;
  * the projection onto the affine dual subspace W -> W_dual (getOptimalDualProjection, certification.cc:323-452) by two
    routes that also return, per element of W_dual, the sum of the absolute values of the terms added on the way to it
    (what a forward error bound gamma_k sum|terms| needs):
      - dual_projection_dense: the oracle as it stands (linear_projection builds A_inv, optimal_dual_projection applies
        it), FP64; A_inv has N(N+1)/2 rows squared, so this route ends near N = 129 (8385^2 doubles);
      - dual_projection_structured: a vectorised restatement in np.longdouble that never builds A_inv (any N).

The structured route.  Column (i, j) of A_inv (certification.cc:538-657) puts x on the diagonal and +- y theta theta on
the rows whose pair shares one index with (i, j).  Collected by ROW (a, c), a < c, with b(p, q) the row of b_W of pair
p < q, R[p] = sum_{j > p} theta_j b(p, j) and C[p] = sum_{i < p} theta_i b(i, p):

    (A_inv b)(a, c) = x b(a, c) + y theta_a (R[c] - C[c]) - y theta_c (R[a] - C[a]) + y (theta_a^2 + theta_c^2) b(a, c)

(the last term returns the two members b(a, c) itself contributes to R[a] and C[c], which the pattern excludes).  The
pairs (p, p + 1), ..., (p, N) are consecutive in the pair list, so every R[p] is a difference of two prefix sums over
that list; C[p] is a scatter-add by the second index.  O(N^2) in all, no loop over pairs.
"""
import numpy as np

from oracle import certifier as C

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps) / 2  # unit round-off of FP64


def gamma(k):
    """gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1)."""
    return k * EPS / (1 - k * EPS)


def dense_minit(R, v1, v2, theta, nb, cbar2):
    N = v1.shape[1]
    npm = 4 + 4 * N
    q = C.rotation_to_quaternion(R)
    thp = np.concatenate([[1.0], theta])
    Q = C.q_cost(v1, v2, nb, cbar2)
    D = C.block_diag_omega(npm, q)
    x = np.kron(thp, q)
    mu = float(x @ (Q @ x))
    J = np.zeros((npm, npm))
    J[:4, :4] = np.eye(4)
    return D.T @ (Q @ D) - mu * J - C.lambda_guess(R, theta, v1, v2, nb, cbar2), mu


def pairs(N1):
    """The pair list (i < j of N1 items) in the order of b_W's rows."""
    return np.triu_indices(N1, 1)


def b_w(W, thp):
    """Rows of b_W (certification.cc:339-378) in longdouble, and per entry the sum of the four |terms|."""
    W = np.asarray(W, dtype=LD)
    th = np.asarray(thp, dtype=LD)
    i, j = pairs(len(th))
    k = np.arange(3)[None, :]
    r0, c0 = (4 * i)[:, None], (4 * j)[:, None]
    Cc, Dd = W[r0 + 3, r0 + k], W[c0 + 3, r0 + k]
    Ee, Ff = W[r0 + 3, c0 + k], W[c0 + 3, c0 + k]
    tij = (th[i] * th[j])[:, None]
    return (-tij * Cc + Dd) + (-Ee + tij * Ff), np.abs(Cc) + np.abs(Dd) + np.abs(Ee) + np.abs(Ff)


def structured_ainv(thp, b, ab):
    """A_inv b without A_inv (module docstring), and |A_inv| ab: per entry the sum of the |terms| of that row."""
    th = np.asarray(thp, dtype=LD)
    N1 = len(th)
    N = N1 - 1
    y = LD(1) / (2 * LD(N) + 6)
    x = (LD(N) + 1) * y
    i, j = pairs(N1)
    start = np.concatenate([[0], np.cumsum(N1 - 1 - np.arange(N1))])  # first pair of row p; start[N1] = all pairs

    def row_col_sums(v, w):
        pre = np.concatenate([np.zeros((1, 3), dtype=LD), np.cumsum(w[j][:, None] * v, axis=0)])
        Rs = pre[start[1:]] - pre[start[:-1]]
        Cs = np.zeros((N1, 3), dtype=LD)
        np.add.at(Cs, j, w[i][:, None] * v)
        return Rs, Cs

    Rs, Cs = row_col_sums(b, th)
    S = Rs - Cs
    ta, tc = th[i][:, None], th[j][:, None]
    out = x * b + y * ta * S[j] - y * tc * S[i] + y * (ta * ta + tc * tc) * b
    Ra, Ca = row_col_sums(ab, np.ones(N1, dtype=LD))
    # (R[a] and C[c] each hold ab(a, c) once; the pattern has it on the diagonal only)
    terms = x * ab + y * (Ra[j] + Ca[j] + Ra[i] + Ca[i] - 2 * ab)
    return out, terms


def assemble(W, thp, y3, ay3):
    """W_dual from W and the rows y3 of A_inv b_W (certification.cc:381-451), and the sum of |terms| per element, given
    those of y3 (ay3).  Longdouble in, longdouble out."""
    W = np.asarray(W, dtype=LD)
    th = np.asarray(thp, dtype=LD)
    N1 = len(th)
    n = 4 * N1
    i, j = pairs(N1)
    B = W.reshape(N1, 4, N1, 4)  # [block row, r, block column, c]
    upper = (np.arange(N1)[:, None] < np.arange(N1)[None, :])[:, None, :, None]
    A = np.where(upper, (B - B.transpose(0, 3, 2, 1)) / 2, LD(0))  # (W_ij - W_ij^T) / 2 of the blocks above the diagonal
    T = np.where(upper, (np.abs(B) + np.abs(B.transpose(0, 3, 2, 1))) / 2, LD(0))
    Wd, Tm = A.reshape(n, n).copy(), T.reshape(n, n).copy()
    k = np.arange(3)[None, :]
    r0, c0 = (4 * i)[:, None], (4 * j)[:, None]
    Wd[r0 + k, c0 + 3], Wd[r0 + 3, c0 + k] = y3, -y3
    Tm[r0 + k, c0 + 3], Tm[r0 + 3, c0 + k] = ay3, ay3
    Wd, Tm = Wd + Wd.T, Tm + Tm.T  # (the diagonal blocks are zero so far)
    # diagonal blocks: last row / column from the block row sums with kron(theta, e4) (getBlockRowSum)
    rs = (Wd[:, 3::4] * th[None, :]).sum(axis=1).reshape(N1, 4)
    rt = Tm[:, 3::4].sum(axis=1).reshape(N1, 4)
    d = np.arange(N1)
    Wb, Tb = Wd.reshape(N1, 4, N1, 4), Tm.reshape(N1, 4, N1, 4)
    diag = B[d, :, d, :].copy()  # [block, r, c]
    dt = np.abs(diag)
    mean = diag[:, :3, :3].sum(axis=0) / N1
    diag[:, :3, :3] -= mean[None]
    dt[:, :3, :3] += (dt[:, :3, :3].sum(axis=0) / N1)[None]
    diag[:, :, 3], dt[:, :, 3] = -th[:, None] * rs, rt
    diag[:, 3, :], dt[:, 3, :] = -th[:, None] * rs, rt
    Wb[d, :, d, :], Tb[d, :, d, :] = diag, dt
    return Wd, Tm


def element_classes(N):
    """Boolean masks over W_dual by the path that leads to an element: 'off33' the 3 x 3 parts and corners of the
    off-diagonal blocks, 'offborder' their last rows / columns, 'diagborder' the last rows / columns of the diagonal blocks
    (corner included), 'diag33' the diagonal blocks' 3 x 3 parts."""
    n = 4 * N + 4
    blk = np.arange(n) // 4
    last = (np.arange(n) % 4) == 3
    same = blk[:, None] == blk[None, :]
    border = last[:, None] ^ last[None, :]
    return dict(off33=~same & ~border, offborder=~same & border, diagborder=same & (last[:, None] | last[None, :]),
                diag33=same & ~last[:, None] & ~last[None, :])


def dual_projection_structured(W, thp):
    """(W_dual, sum|terms|), both longdouble, without A_inv."""
    b, ab = b_w(W, thp)
    return assemble(W, thp, *structured_ainv(thp, b, ab))


def dual_projection_dense(W, thp):
    """(W_dual, sum|terms|): the oracle's dense route as it stands (FP64), the term sums through |A_inv|."""
    thp = np.asarray(thp, dtype=np.float64)
    A_inv = C.linear_projection(thp)
    Wd = C.optimal_dual_projection(np.asarray(W, dtype=np.float64), thp, A_inv)
    _, ab = b_w(W, thp)
    ay = np.abs(A_inv) @ ab.astype(np.float64)
    _, Tm = assemble(W, thp, np.zeros_like(ab), ay.astype(LD))
    return Wd, Tm
