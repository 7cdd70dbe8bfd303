"""A vectorised numpy restatement of the tuple-test contract (include/teaser_hip.h, "tuple_test_batch"), and the
problems the tuple-test tests share.  test_tuple_test_reference.py pins it to the host function
(teaser_hip_tuple_test, the specification); the GPU tests compare the batched call with that host function."""
import functools

import numpy as np

_GAMMA, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_CHUNK = 1 << 20  # trials per vectorised step


def draws(seed, m):
    """splitmix64's m-th output (m >= 1, a uint64 array) for `seed`: the state after m draws is seed + m gamma."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + m * _GAMMA
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def _side(p, a, b):
    d = p[a] - p[b]  # float32 throughout: every operation rounded once, the squares summed in x, y, z order
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def tuple_test(src, dst, pairs, tuple_scale, seed):
    """The surviving pairs as a k x 2 int32 array (sorted, unique); seed must not be 0 (the clock)."""
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 3)
    dst = np.ascontiguousarray(dst, dtype=np.float32).reshape(-1, 3)
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    ncorr, s = len(pairs), np.float32(tuple_scale)
    if not s > 0 or ncorr == 0:
        return pairs.copy()  # untouched: neither sorted nor made unique
    if seed == 0:
        raise ValueError("seed 0 means the clock: nothing to restate")
    if (pairs < 0).any() or (pairs[:, 0] >= len(src)).any() or (pairs[:, 1] >= len(dst)).any():
        raise ValueError("a pair's index lies outside its cloud")
    keep = np.zeros(ncorr, dtype=bool)
    for lo in range(0, 100 * ncorr, _CHUNK):
        i = np.arange(lo, min(lo + _CHUNK, 100 * ncorr), dtype=np.uint64)
        r = [(draws(seed, np.uint64(3) * i + np.uint64(k + 1)) % np.uint64(ncorr)).astype(np.int64) for k in range(3)]
        ok = np.ones(len(i), dtype=bool)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            li = _side(src, pairs[r[a], 0], pairs[r[b], 0])
            lj = _side(dst, pairs[r[a], 1], pairs[r[b], 1])
            ok &= (li * s < lj) & (lj < li / s)
        for k in range(3):
            keep[r[k][ok]] = True
    return np.unique(pairs[keep], axis=0).reshape(-1, 2)


def as_array(host_pairs):
    """tp.tuple_test's list of tuples as the k x 2 int32 array the batched calls return."""
    return np.asarray(host_pairs, dtype=np.int32).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def scene():
    """The scene of test_features_oracle.py::test_tuple_constraint_host_function: 400 points, a rotation of 0.7 rad
    about z, 200 consistent pairs and ~120 random ones; (src, dst, the 320 sorted pairs as an int32 array)."""
    rng = np.random.default_rng(5)
    n = 400
    src = rng.random((n, 3)).astype(np.float32)
    th = 0.7
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    dst = (src @ R.T + np.array([0.3, -0.2, 0.1])).astype(np.float32)
    good = [(i, i) for i in range(0, 200)]
    bad = [(i, int(rng.integers(0, n))) for i in range(200, 320)]
    bad = [(a, b) for a, b in bad if a != b]
    pairs = np.array(sorted(set(good + bad)), dtype=np.int32)
    for a in (src, dst, pairs):
        a.setflags(write=False)
    return src, dst, pairs


SCALE = 0.95  # the scene's tuple scale


def reversed_with_repeats():
    """The scene's pair list reversed, its first ten pairs appended once more: unsorted, with repeats."""
    pairs = scene()[2]
    return np.ascontiguousarray(np.concatenate([pairs[::-1], pairs[:10]]))


def coincident_scene():
    """The scene with points 0 and 1 made coincident in both clouds (a side of length 0 wherever both are drawn)."""
    src, dst, pairs = scene()
    src, dst = src.copy(), dst.copy()
    src[1], dst[1] = src[0], dst[0]
    return src, dst, pairs


@functools.lru_cache(maxsize=None)
def large_problem():
    """40 003 pairs on a random unit-cube cloud mapped onto itself: odd i to itself, even i through a permutation.
    4 000 300 trials: the grid stride, and draws whose 64-bit remainder differs from any 32-bit shortcut."""
    rng = np.random.default_rng(40003)
    n = 40003
    cloud = rng.random((n, 3)).astype(np.float32)
    to = np.arange(n)
    even = np.arange(0, n, 2)
    to[even] = even[rng.permutation(len(even))]
    pairs = np.stack([np.arange(n), to], axis=1).astype(np.int32)
    for a in (cloud, pairs):
        a.setflags(write=False)
    return cloud, cloud, pairs
