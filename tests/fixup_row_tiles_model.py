"""CPU model of what the K1 filter hands to the fix-up, for tests/test_gpu_fixup_row_tiles.py: the flagged lane-tiles
(group items) per cell (row tile, column chunk) of the region arena (csrc/fixup_regions.h), from the band model of
tests/test_k1_f16_band_model.py (`operands`, one f32 accumulation order) and the device's own constants
(csrc/k1_consts.h through tests/k1_f16_host.py).  The device adds in another order, so a regime is asserted with a
factor of two over its threshold.  Also the input of the n = 1100 case: an `adversarial` cloud with one row tile's
points moved so that the tile has no item."""
import numpy as np

from k1_f16_host import host_consts
from test_k1_f16_band_model import accumulate, adversarial, f32, operands

CHUNK_TILES = 8      # column tiles of a chunk (fxr::kChunkTiles)
REGION_ITEMS = 63    # items of a region (fxr::kRegionItems)
ROUND_ITEMS = 64     # items of one queue round of the fix-up
WAVE_BUFFER = 384    # kWorkBuf: items a K1 wave can stage per chunk (more -> the batch reruns on the FP64 kernel)


def n_chunks(T):
    return (T + CHUNK_TILES - 1) // CHUNK_TILES


def band(src, dst, beta):
    """src, dst [n, 3] -> (operands, C, admitted) with the device's constants"""
    op = operands(src, dst, beta)
    kc = host_consts([(beta, op["s"], op["r2"])])[0]
    return op, float(kc["C"]), kc["use_mfma"] == 1


def min_abs_d(src, dst, beta):
    """[T, 4, n] float: per row tile, row group g = 2 rt + h (the 16 rows 32 rt + 4 h + (q & 3) + 8 (q >> 2) of a lane-tile)
    and column, the smallest |d~| of the group's pairs as K1 sees them -- rows beyond n are copies of the last point,
    a group whose first row lies beyond n is dropped (inf), the pair of a point with itself is left out, columns left of
    the row tile's diagonal tile are not computed (inf); plus C and the admission flag"""
    n = len(src)
    T = (n + 63) // 64
    op, C, adm = band(src, dst, beta)
    A, B = op["A"].astype(np.float64), op["B"].astype(np.float64)
    out = np.full((T, 4, n), np.inf)
    cols = np.arange(n)
    for I in range(T):
        rows = np.minimum(64 * I + np.arange(64), n - 1)
        Pu = A[rows, None, :32] * B[None, :, :]       # [64, n, 32] exact products
        Pw = A[rows, None, 32:] * B[None, :, :16]
        u = accumulate(Pu.reshape(-1, 32), range(32))
        w = accumulate(Pw.reshape(-1, 16), range(16))
        d = (u.astype(np.float64) * u.astype(np.float64) + w.astype(np.float64)).astype(f32)
        ad = np.abs(d.astype(np.float64)).reshape(64, n)
        ad[(64 * I + np.arange(64))[:, None] == cols[None, :]] = np.inf   # the lane's own pair
        ad[:, cols < 64 * I] = np.inf                                       # left of the diagonal tile
        local = np.arange(64)
        grp = 2 * (local >> 5) + ((local >> 2) & 1)
        for g in range(4):
            first = 64 * I + 32 * (g >> 1) + 4 * (g & 1)
            if first < n:
                out[I, g] = ad[grp == g].min(0)
    return out, C, adm


def items_per_cell(mins, thr):
    """[T, n_chunks] int: lane-tiles with min |d~| <= thr per (row tile, column chunk)"""
    T, _, n = mins.shape
    nch = n_chunks(T)
    cnt = np.zeros((T, nch), int)
    flagged = mins <= thr
    for Xc in range(nch):
        cnt[:, Xc] = flagged[:, :, 512 * Xc:min(512 * (Xc + 1), n)].sum((1, 2))
    return cnt


ENGINEERED_BETA = 0.09


def engineered_1100(seed, beta=ENGINEERED_BETA):
    """n = 1100 (18 row tiles, 3 column chunks): an `adversarial` cloud -- every point an inlier displaced by about
    beta, so that 5 - 8 % of the lane-tiles are group items: regions with more than 63 items and row tiles with more
    than one queue round come by themselves -- in which the points of row tile 5 (320 .. 383) are moved: their src
    images into a ball of 1e-3 at the centre, their dst images onto a 4 x 4 x 4 lattice of spacing 0.3 at distance 3.6.
    For every partner j then |d_j - d_i| - |s_j - s_i| >= 0.2 = 2.2 beta (inside the tile 0.3 - 0.004), far outside the
    band: the tile has no item.  (beta = 0.09 and the distance are chosen so that the wider bounding box -- one bit of
    the normalisation -- does not push a K1 wave beyond its 384 staged items per chunk, which would send the batch to
    the FP64 rerun and test nothing: asserted by the test.)"""
    rng = np.random.default_rng(seed)
    n = 1100
    src, dst = adversarial(rng, n, 1.0, beta)
    far = np.arange(320, 384)
    src[far] = rng.uniform(-1e-3, 1e-3, size=(64, 3))
    lattice = np.stack(np.meshgrid(*[np.arange(4) - 1.5] * 3, indexing="ij"), -1).reshape(64, 3) * 0.3
    dst[far] = np.array([3.6, 0.0, 0.0]) + lattice
    return src, dst
