"""A numpy model of the degree closure's three-launch route (csrc/kernels_graph.hip: tim_closure_pairs_kernel,
csrc/closure_h.h: the H rule the verdict launch applies), and the cases its tests share.

The pair kernel: a wave takes a 64 x 64 block (A, B >= A) of rank pairs.  Lane l holds column rank 64 B + l for the
whole row loop; row r of the loop gives one ballot -- the row word (64 A + r, B) -- and lane l ORs its own predicate bit
into bit r of a column word, which is the mirrored word (64 B + l, A).  The predicate is masked by
`64 B + l < m and 64 A + r < 64 B + l`.  Off the diagonal both words are stored, on it their OR."""
import functools

import numpy as np

CORE_CAP = 2048
SIZES = (2, 3, 63, 64, 65, 127, 128, 129, 1000, 2048)
GRIDS = (1, 16, 64)


def random_symmetric(m, density, seed):
    rng = np.random.default_rng(seed)
    up = np.triu(rng.random((m, m)) < density, 1)
    return up | up.T


def bench_like(m, seed):
    """A clique on ~55 % of the ranks (the inliers) under a sparse random rest, the vertices then ranked by degree
    descending: what the headline workload hands to the closure."""
    rng = np.random.default_rng(seed)
    adj = random_symmetric(m, 0.08, seed + 1)
    inl = rng.permutation(m)[: max(2, (55 * m) // 100)]
    adj[np.ix_(inl, inl)] = True
    np.fill_diagonal(adj, False)
    deg = adj.sum(1) + rng.integers(0, 40, m)  # (edges to vertices outside R)
    order = np.lexsort((np.arange(m), -deg))
    return adj[np.ix_(order, order)], deg[order]


@functools.lru_cache(maxsize=None)
def case(m, kind):
    """(adjacency by rank [m][m] bool, clamped degrees by rank [m], not increasing)"""
    if kind == "bench":
        adj, deg = bench_like(m, 1000 + m)
    else:
        density = {"sparse": 0.05, "half": 0.5, "dense": 0.95}[kind]
        adj = random_symmetric(m, density, 7 * m + len(kind))
        rng = np.random.default_rng(m + 17)
        # any sequence that does not increase: between "all P below d" and "all P above d", with runs of equal degrees
        deg = np.sort(rng.integers(0, 2 * m + 2, m) // 3 * 3)[::-1]
    deg = np.minimum(deg, CORE_CAP).astype(np.int64)
    assert np.all(np.diff(deg) <= 0) and not adj.diagonal().any() and (adj == adj.T).all()
    adj.setflags(write=False)
    deg.setflags(write=False)
    return adj, deg


KINDS = ("sparse", "half", "dense", "bench")


def pack_words(bits):
    """[..., 64] bool -> uint64, bit k = element k"""
    return (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def pairs_launch(adj, grid):
    """The pair kernel on a grid of `grid` workgroups of four waves: (pool [CORE_CAP][CORE_CAP / 64] uint64, the number
    of stores every word has received)."""
    m = adj.shape[0]
    ng = (m + 63) // 64
    pool = np.zeros((CORE_CAP, CORE_CAP // 64), np.uint64)
    writes = np.zeros(pool.shape, np.int64)
    units = [(A, B) for A in range(ng) for B in range(A, ng)]
    lane = np.arange(64)
    for wv in range(4 * grid):  # wave wv = 4 * workgroup + wave in it
        for u in range(wv, len(units), 4 * grid):
            A, B = units[u]
            ra, rb = 64 * A + lane, 64 * B + lane
            rows = min(64, m - 64 * A)
            e = adj[np.ix_(64 * A + np.arange(rows), np.minimum(rb, m - 1))]  # [r][l]
            valid = (rb[None, :] < m) & ((64 * A + np.arange(rows))[:, None] < rb[None, :])
            p = np.zeros((64, 64), bool)
            p[:rows] = e & valid
            word = pack_words(p)      # lane r: the ballot of row r
            colw = pack_words(p.T)    # lane l: its own bit of every row r at position r
            if A == B:
                ok = ra < m
                pool[ra[ok], A] = (word | colw)[ok]
                writes[ra[ok], A] += 1
            else:
                ok = ra < m
                pool[ra[ok], B] = word[ok]
                writes[ra[ok], B] += 1
                ok = rb < m
                pool[rb[ok], A] = colw[ok]
                writes[rb[ok], A] += 1
    return pool, writes


def unpack_rows(pool, m):
    ng = (m + 63) // 64
    bits = (pool[:m, :ng, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(m, 64 * ng)[:, :m].astype(bool)


def h_definition(adj, deg):
    """H(v) = max over the set bits i of row v of min(P_i, d_i), P_i = the set bits up to and including i"""
    out = np.zeros(adj.shape[0], np.int64)
    for v, row in enumerate(adj):
        idx = np.flatnonzero(row)
        if idx.size:
            out[v] = np.minimum(np.arange(1, idx.size + 1), deg[idx]).max()
    return out


def _popc(x):
    return bin(x).count("1")


def _ctz(x):
    return (x & -x).bit_length() - 1


def h_block(full, base, cols, dblk, hmax):
    """csrc/closure_h.h, clh::block, restated"""
    if full == 0:
        return hmax
    cnt = _popc(full)
    if base + cnt <= dblk[cols - 1]:
        cand = base + cnt
    elif base + 1 >= dblk[0]:
        cand = dblk[_ctz(full)]
    else:
        lo, hi = 0, cols
        while lo < hi:
            mid = (lo + hi) >> 1
            if base + _popc(full & ((1 << (mid + 1)) - 1)) >= dblk[mid]:
                hi = mid
            else:
                lo = mid + 1
        front, back = full & ((1 << lo) - 1), full & ~((1 << lo) - 1)
        cand = base + _popc(front) if front else 0
        if back:
            cand = max(cand, dblk[_ctz(back)])
    return max(hmax, cand)


def h_from_rows(pool, m, deg):
    ng = (m + 63) // 64
    deg = [int(x) for x in deg]
    out = np.zeros(m, np.int64)
    for v in range(m):
        base = hmax = 0
        for B in range(ng):
            w = int(pool[v, B])
            hmax = h_block(w, base, min(64, m - 64 * B), deg[64 * B:64 * B + 64], hmax)
            base += _popc(w)
        out[v] = hmax
    return out
