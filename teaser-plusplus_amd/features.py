"""The batched correspondence front-end on the GPU: FPFH descriptors and mutual-nearest-neighbour matching for many
clouds / pairs per call -- ``compute_fpfh_batch``, ``match_features_batch`` and ``correspondences_batch`` (clouds in,
correspondences out, the features staying on the device in between).  The arithmetic is that of
``FPFHEstimation.computeFPFHFeatures`` / ``Matcher.calculateCorrespondences`` bit for bit; the contract is written out
in include/teaser_hip.h ("Batched correspondence front-end").  ``knn_features_batch``, ``match_features_knn_batch`` and
``correspondences_knn_batch`` (and their single-problem forms) match every point with its k nearest descriptors, as
the reference's tutorial does with a host KD-tree; their semantics are in the same header ("k nearest").
``tuple_test_batch`` runs the matcher's tuple constraint for many problems in one launch sequence, with the results of
the host routine ``tuple_test`` (same header, "tuple_test_batch"); the correspondence calls take ``tuple_scale``.

One library handle is kept per device between calls; calls from several threads are safe -- each handle has a lock,
so calls for one device run one after the other.  device=-1 means the calling thread's current HIP device at the
time of the call.  Without a GPU the calls raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C

import numpy as np

from ._handles import Handle, HandleCache, _cloud

_vp, _ip, _fp, _dp, _i64p = (C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double),
                             C.POINTER(C.c_int64))
_u64p = C.POINTER(C.c_uint64)


def declare(L):
    """ctypes signatures of the front-end entry points (called by the package's lib())."""
    L.teaser_hip_features_create.argtypes = [C.c_int32, C.POINTER(_vp)]
    L.teaser_hip_features_destroy.argtypes = [_vp]
    L.teaser_hip_features_last_error.argtypes = [_vp]
    L.teaser_hip_features_last_error.restype = C.c_char_p
    L.teaser_hip_features_fill_scratch.argtypes = [_vp, C.c_int32, C.POINTER(C.c_int64)]
    L.teaser_hip_features_set_budgets.argtypes = [_vp, C.c_int64, C.c_int64]
    L.teaser_hip_features_fpfh_batch.argtypes = [_vp, C.c_int32, C.POINTER(_fp), _ip, _dp, _dp, C.POINTER(_fp),
                                                 C.POINTER(_fp)]
    L.teaser_hip_features_match_batch.argtypes = [_vp, C.c_int32, C.POINTER(_fp), _ip, C.POINTER(_fp), _ip, C.c_int32,
                                                  C.c_int32, C.POINTER(_ip), _i64p, _i64p]
    L.teaser_hip_features_correspondences_batch.argtypes = [
        _vp, C.c_int32, C.POINTER(_fp), _ip, C.POINTER(_fp), _ip, _dp, _dp, C.c_int32, C.POINTER(_ip), _i64p, _i64p,
        C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp)]
    L.teaser_hip_features_knn_batch.argtypes = [_vp, C.c_int32, C.POINTER(_fp), _ip, C.POINTER(_fp), _ip, C.c_int32,
                                                C.c_int32, C.POINTER(_ip), C.POINTER(_fp)]
    L.teaser_hip_features_match_knn_batch.argtypes = [_vp, C.c_int32, C.POINTER(_fp), _ip, C.POINTER(_fp), _ip,
                                                      C.c_int32, C.c_int32, C.c_int32, C.POINTER(_ip), _i64p, _i64p]
    L.teaser_hip_features_correspondences_knn_batch.argtypes = [
        _vp, C.c_int32, C.POINTER(_fp), _ip, C.POINTER(_fp), _ip, _dp, _dp, C.c_int32, C.c_int32, C.POINTER(_ip), _i64p,
        _i64p, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp)]
    L.teaser_hip_features_tuple_test_batch.argtypes = [_vp, C.c_int32, C.POINTER(_fp), _ip, C.POINTER(_fp), _ip, _fp,
                                                       _u64p, C.POINTER(_ip), _i64p]


class _Handle(Handle):
    def _set_budget(self, list_bytes=None, part_bytes=None):
        """Test hook: the budgets of one wave in bytes (None or <= 0: the default) -- list_bytes for the neighbour lists
        of a wave of clouds, part_bytes for the partial nearest-neighbour results of a wave of pairs (and the pairs of
        a wave of tuple-test problems).  Small values
        split a call into many waves; results do not depend on them."""
        with self.lock:
            self._lib.teaser_hip_features_set_budgets(self.h, int(list_bytes or 0), int(part_bytes or 0))


_cache = HandleCache("teaser_hip_features", _Handle)
_handle = _cache.get


# ---- argument normalisation (no device needed) ----------------------------------------------------------------------
def _clouds(clouds, what="clouds"):
    """A list of n_b x 3 float32 C-contiguous arrays (an empty cloud is 0 x 3)."""
    return [_cloud(c, "%s[%d]" % (what, k), np.float32) for k, c in enumerate(clouds)]


def _per_problem(v, batch, what, dtype):
    """One `dtype` value per problem from a scalar or a sequence of `batch` values."""
    a = np.asarray(v, dtype=dtype)
    if a.ndim == 0:
        return np.full(max(batch, 1), a)
    if a.shape != (batch,):
        raise ValueError("%s must be a scalar or one value per problem (%d), got shape %s" % (what, batch, a.shape))
    return np.ascontiguousarray(a) if batch else np.zeros(1, dtype=dtype)


def _radii(r, batch, what):
    return _per_problem(r, batch, what, np.float64)


def _features(feats, what):
    """A list of n_b x dim float32 C-contiguous arrays and their common dim (None when every array is empty)."""
    out, dim = [], None
    for k, f in enumerate(feats):
        a = np.ascontiguousarray(np.asarray(f, dtype=np.float32))
        if a.ndim != 2:
            if a.size:
                raise ValueError("%s[%d] must be an n x dim array, got shape %s" % (what, k, a.shape))
            a = a.reshape(0, 0)
        if a.shape[0] and a.shape[1]:
            if dim is not None and a.shape[1] != dim:
                raise ValueError("%s[%d] has dim %d, earlier features have dim %d" % (what, k, a.shape[1], dim))
            dim = a.shape[1]
        out.append(a)
    return out, dim


def _same_length(a, b, what_a, what_b):
    if len(a) != len(b):
        raise ValueError("%s and %s must have the same length, got %d and %d" % (what_a, what_b, len(a), len(b)))


def _ptrs(arrays, ty):
    """A ctypes array of pointers to the arrays (at least one slot, so that an empty batch still has an address)."""
    return (ty * max(len(arrays), 1))(*[a.ctypes.data_as(ty) for a in arrays])


def _counts(arrays):
    return np.array([a.shape[0] for a in arrays] or [0], dtype=np.int32)


def _pair_buffers(n_src, n_dst, batch):
    cap = np.array([int(n_src[b]) + int(n_dst[b]) for b in range(batch)] or [0], dtype=np.int64)
    bufs = [np.zeros((max(int(cap[b]), 1), 2), dtype=np.int32) for b in range(batch)]
    return cap, bufs, np.zeros(max(batch, 1), dtype=np.int64)


KNN_MAX = 16  # TEASER_HIP_FEATURES_KNN_MAX


def _knn_k(k):
    """k as an int in [1, KNN_MAX]; anything else (a float, a bool, 0, 17) is a ValueError naming k."""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= KNN_MAX:
        raise ValueError("k must be an integer in [1, %d], got %r" % (KNN_MAX, k))
    return int(k)


def _two_sides(a_feats, b_feats, what_a, what_b):
    """Two lists of feature arrays of one length and one dim: (arrays a, arrays b, dim)."""
    _same_length(a_feats, b_feats, what_a, what_b)
    a, dim_a = _features(a_feats, what_a)
    d, dim_d = _features(b_feats, what_b)
    if dim_a is not None and dim_d is not None and dim_a != dim_d:
        raise ValueError("%s have dim %d, %s have dim %d" % (what_a, dim_a, what_b, dim_d))
    return a, d, dim_a or dim_d or 33


def _knn_pair_buffers(n_src, n_dst, k, batch):
    cap = np.array([int(n_src[b]) * min(k, int(n_dst[b])) for b in range(batch)] or [0], dtype=np.int64)
    bufs = [np.zeros((max(int(cap[b]), 1), 2), dtype=np.int32) for b in range(batch)]
    return cap, bufs, np.zeros(max(batch, 1), dtype=np.int64)


# ---- the calls ------------------------------------------------------------------------------------------------------
def compute_fpfh_batch(clouds, normal_radius, fpfh_radius, device=-1, return_normals=False):
    """FPFH of many clouds (mixed sizes allowed) in one launch sequence.  clouds: list of n_b x 3 arrays; the radii:
    one value for all clouds or one per cloud.  Returns the list of n_b x 33 float32 features -- with
    return_normals=True the tuple (features, normals), normals being the list of n_b x 3 float32 PCL-semantics normals.
    Each result is bit-identical to FPFHEstimation.computeFPFHFeatures on the same cloud alone."""
    pts = _clouds(clouds)
    b = len(pts)
    nr, fr = _radii(normal_radius, b, "normal_radius"), _radii(fpfh_radius, b, "fpfh_radius")
    n = _counts(pts)
    out = [np.zeros((p.shape[0], 33), dtype=np.float32) for p in pts]
    nrm = [np.zeros((p.shape[0], 3), dtype=np.float32) for p in pts] if return_normals else None
    h = _handle(device)
    h.call(h._lib.teaser_hip_features_fpfh_batch, b, _ptrs(pts, _fp), n.ctypes.data_as(_ip), nr.ctypes.data_as(_dp),
           fr.ctypes.data_as(_dp), _ptrs(out, _fp), None if nrm is None else _ptrs(nrm, _fp))
    return (out, nrm) if return_normals else out


def match_features_batch(src_feats, dst_feats, use_crosscheck=True, device=-1):
    """Matcher.calculateCorrespondences (use_tuple_test=False) for many feature pairs in one launch sequence: per
    pair the k_b x 2 int32 array of sorted unique (src, dst) index pairs."""
    _same_length(src_feats, dst_feats, "src_feats", "dst_feats")
    a, dim_a = _features(src_feats, "src_feats")
    d, dim_d = _features(dst_feats, "dst_feats")
    if dim_a is not None and dim_d is not None and dim_a != dim_d:
        raise ValueError("src_feats have dim %d, dst_feats have dim %d" % (dim_a, dim_d))
    dim = dim_a or dim_d or 33
    b = len(a)
    n_src, n_dst = _counts(a), _counts(d)
    cap, bufs, cnt = _pair_buffers(n_src, n_dst, b)
    h = _handle(device)
    h.call(h._lib.teaser_hip_features_match_batch, b, _ptrs(a, _fp), n_src.ctypes.data_as(_ip), _ptrs(d, _fp),
           n_dst.ctypes.data_as(_ip), dim, 1 if use_crosscheck else 0, _ptrs(bufs, _ip), cap.ctypes.data_as(_i64p),
           cnt.ctypes.data_as(_i64p))
    return [bufs[k][:int(cnt[k])].copy() for k in range(b)]


def correspondences_batch(src_clouds, dst_clouds, normal_radius, fpfh_radius, use_crosscheck=True, tuple_scale=0.0,
                          tuple_seed=0, return_features=False, return_normals=False, device=-1):
    """Clouds in, correspondences out, for many pairs in one launch sequence: FPFH of both clouds of every pair, then
    the mutual nearest-neighbour matching, with the features staying on the device in between.  Returns the list of
    k_b x 2 int32 arrays of (src, dst) pairs; with return_features / return_normals a tuple
    (pairs, [src_feats, dst_feats], [src_normals, dst_normals]) holding the parts asked for.  tuple_scale != 0 applies
    the tuple test to all pairs in one more launch sequence (tuple_test_batch, seeded by tuple_seed; one value or one
    per pair each)."""
    _same_length(src_clouds, dst_clouds, "src_clouds", "dst_clouds")
    sp, dp = _clouds(src_clouds, "src_clouds"), _clouds(dst_clouds, "dst_clouds")
    b = len(sp)
    nr, fr = _radii(normal_radius, b, "normal_radius"), _radii(fpfh_radius, b, "fpfh_radius")
    n_src, n_dst = _counts(sp), _counts(dp)
    cap, bufs, cnt = _pair_buffers(n_src, n_dst, b)
    feats = nrms = None
    if return_features:
        feats = [[np.zeros((p.shape[0], 33), dtype=np.float32) for p in side] for side in (sp, dp)]
    if return_normals:
        nrms = [[np.zeros((p.shape[0], 3), dtype=np.float32) for p in side] for side in (sp, dp)]
    h = _handle(device)
    h.call(h._lib.teaser_hip_features_correspondences_batch, b, _ptrs(sp, _fp), n_src.ctypes.data_as(_ip),
           _ptrs(dp, _fp), n_dst.ctypes.data_as(_ip), nr.ctypes.data_as(_dp), fr.ctypes.data_as(_dp),
           1 if use_crosscheck else 0, _ptrs(bufs, _ip), cap.ctypes.data_as(_i64p), cnt.ctypes.data_as(_i64p),
           None if feats is None else _ptrs(feats[0], _fp), None if feats is None else _ptrs(feats[1], _fp),
           None if nrms is None else _ptrs(nrms[0], _fp), None if nrms is None else _ptrs(nrms[1], _fp))
    pairs = [bufs[k][:int(cnt[k])].copy() for k in range(b)]
    if np.any(tuple_scale):
        pairs = tuple_test_batch(sp, dp, pairs, tuple_scale, tuple_seed, device)
    parts = [pairs] + ([feats] if return_features else []) + ([nrms] if return_normals else [])
    return parts[0] if len(parts) == 1 else tuple(parts)


# ---- k nearest neighbours (include/teaser_hip.h, "k nearest") -------------------------------------------------------
def knn_features_batch(data, query, k, return_distance=False, device=-1):
    """The raw search for many problems in one launch sequence: per problem the n_query x k int32 array of the k
    nearest rows of data[b] for every row of query[b], in ascending (squared L2 distance in float, index) order --
    ties go to the lower index; slots beyond min(k, n_data) hold -1.  With return_distance=True the tuple
    (indices, distances), distances being the list of n_query x k float32 squared distances (+inf in unused slots)."""
    k = _knn_k(k)
    dat, qry, dim = _two_sides(data, query, "data", "query")
    b = len(dat)
    n_d, n_q = _counts(dat), _counts(qry)
    idx = [np.zeros((q.shape[0], k), dtype=np.int32) for q in qry]
    dist = [np.zeros((q.shape[0], k), dtype=np.float32) for q in qry] if return_distance else None
    h = _handle(device)
    h.call(h._lib.teaser_hip_features_knn_batch, b, _ptrs(dat, _fp), n_d.ctypes.data_as(_ip), _ptrs(qry, _fp),
           n_q.ctypes.data_as(_ip), dim, k, _ptrs(idx, _ip), None if dist is None else _ptrs(dist, _fp))
    return (idx, dist) if return_distance else idx


def match_features_knn_batch(src_feats, dst_feats, k, mutual=True, device=-1):
    """k-nearest-neighbour matching of many feature pairs in one launch sequence: per pair the sorted (src, dst) int32
    pairs (i, j) with j among the k nearest target rows of source row i -- with mutual=True only those where i is also
    among the k nearest source rows of j.  k = 1, mutual=True equals match_features_batch(use_crosscheck=True);
    mutual=False is the tutorial's one-directional set, not the reference matcher's two-directional union."""
    k = _knn_k(k)
    a, d, dim = _two_sides(src_feats, dst_feats, "src_feats", "dst_feats")
    b = len(a)
    n_src, n_dst = _counts(a), _counts(d)
    cap, bufs, cnt = _knn_pair_buffers(n_src, n_dst, k, b)
    h = _handle(device)
    h.call(h._lib.teaser_hip_features_match_knn_batch, b, _ptrs(a, _fp), n_src.ctypes.data_as(_ip), _ptrs(d, _fp),
           n_dst.ctypes.data_as(_ip), dim, k, 1 if mutual else 0, _ptrs(bufs, _ip), cap.ctypes.data_as(_i64p),
           cnt.ctypes.data_as(_i64p))
    return [bufs[p][:int(cnt[p])].copy() for p in range(b)]


def correspondences_knn_batch(src_clouds, dst_clouds, normal_radius, fpfh_radius, k, mutual=True,
                              return_features=False, return_normals=False, device=-1, tuple_scale=0.0, tuple_seed=0):
    """Clouds in, k-nearest-neighbour correspondences out, for many pairs in one launch sequence: compute_fpfh_batch
    followed by match_features_knn_batch with the features staying on the device.  Returns as correspondences_batch
    does: the list of pair arrays, or a tuple with [src_feats, dst_feats] / [src_normals, dst_normals] where asked.
    tuple_scale != 0 then applies the tuple test to all pairs (tuple_test_batch, seeded by tuple_seed)."""
    k = _knn_k(k)
    _same_length(src_clouds, dst_clouds, "src_clouds", "dst_clouds")
    sp, dp = _clouds(src_clouds, "src_clouds"), _clouds(dst_clouds, "dst_clouds")
    b = len(sp)
    nr, fr = _radii(normal_radius, b, "normal_radius"), _radii(fpfh_radius, b, "fpfh_radius")
    n_src, n_dst = _counts(sp), _counts(dp)
    cap, bufs, cnt = _knn_pair_buffers(n_src, n_dst, k, b)
    feats = nrms = None
    if return_features:
        feats = [[np.zeros((p.shape[0], 33), dtype=np.float32) for p in side] for side in (sp, dp)]
    if return_normals:
        nrms = [[np.zeros((p.shape[0], 3), dtype=np.float32) for p in side] for side in (sp, dp)]
    h = _handle(device)
    h.call(h._lib.teaser_hip_features_correspondences_knn_batch, b, _ptrs(sp, _fp), n_src.ctypes.data_as(_ip),
           _ptrs(dp, _fp), n_dst.ctypes.data_as(_ip), nr.ctypes.data_as(_dp), fr.ctypes.data_as(_dp), k,
           1 if mutual else 0, _ptrs(bufs, _ip), cap.ctypes.data_as(_i64p), cnt.ctypes.data_as(_i64p),
           None if feats is None else _ptrs(feats[0], _fp), None if feats is None else _ptrs(feats[1], _fp),
           None if nrms is None else _ptrs(nrms[0], _fp), None if nrms is None else _ptrs(nrms[1], _fp))
    pairs = [bufs[p][:int(cnt[p])].copy() for p in range(b)]
    if np.any(tuple_scale):
        pairs = tuple_test_batch(sp, dp, pairs, tuple_scale, tuple_seed, device)
    parts = [pairs] + ([feats] if return_features else []) + ([nrms] if return_normals else [])
    return parts[0] if len(parts) == 1 else tuple(parts)


def tuple_test_batch(src_clouds, dst_clouds, pairs, tuple_scale, seed=0, device=-1):
    """The tuple constraint of Matcher::advancedMatching (matcher.cc:223-283) for many problems in one launch sequence:
    per problem the k_b x 2 int32 array of the surviving (src, dst) pairs, sorted and unique -- for a non-zero seed
    exactly what the host routine tuple_test returns for that problem.  pairs: per problem an m_b x 2 array of indices
    into its clouds (unsorted and repeated pairs allowed); tuple_scale and seed: one value for all problems or one per
    problem.  A problem with tuple_scale <= 0 or without pairs comes back untouched; seed 0 seeds from the clock, read
    once per call."""
    _same_length(src_clouds, dst_clouds, "src_clouds", "dst_clouds")
    _same_length(src_clouds, pairs, "src_clouds", "pairs")
    sp, dp = _clouds(src_clouds, "src_clouds"), _clouds(dst_clouds, "dst_clouds")
    b = len(sp)
    bufs = []
    for k, p in enumerate(pairs):
        a = np.array(p, dtype=np.int32)  # (a copy: the call works in place)
        if a.size and (a.ndim != 2 or a.shape[1] != 2):
            raise ValueError("pairs[%d] must be an m x 2 array, got shape %s" % (k, a.shape))
        bufs.append(np.ascontiguousarray(a.reshape(-1, 2)))
    scale = _per_problem(tuple_scale, b, "tuple_scale", np.float32)
    seeds = _per_problem(seed, b, "seed", np.uint64)
    n_src, n_dst = _counts(sp), _counts(dp)
    cnt = np.array([a.shape[0] for a in bufs] or [0], dtype=np.int64)
    h = _handle(device)
    h.call(h._lib.teaser_hip_features_tuple_test_batch, b, _ptrs(sp, _fp), n_src.ctypes.data_as(_ip), _ptrs(dp, _fp),
           n_dst.ctypes.data_as(_ip), scale.ctypes.data_as(_fp), seeds.ctypes.data_as(_u64p), _ptrs(bufs, _ip),
           cnt.ctypes.data_as(_i64p))
    return [bufs[k][:int(cnt[k])].copy() for k in range(b)]


def knn_features(data, query, k, return_distance=False, device=-1):
    """knn_features_batch for one problem: the n_query x k index array (and the distance array)."""
    out = knn_features_batch([data], [query], k, return_distance, device)
    return (out[0][0], out[1][0]) if return_distance else out[0]


def match_features_knn(src_feats, dst_feats, k, mutual=True, device=-1):
    """match_features_knn_batch for one pair: its array of (src, dst) pairs."""
    return match_features_knn_batch([src_feats], [dst_feats], k, mutual, device)[0]


def correspondences_knn(src_cloud, dst_cloud, normal_radius, fpfh_radius, k, mutual=True, device=-1, tuple_scale=0.0,
                        tuple_seed=0):
    """correspondences_knn_batch for one pair: its array of (src, dst) pairs."""
    return correspondences_knn_batch([src_cloud], [dst_cloud], normal_radius, fpfh_radius, k, mutual, device=device,
                                     tuple_scale=tuple_scale, tuple_seed=tuple_seed)[0]
