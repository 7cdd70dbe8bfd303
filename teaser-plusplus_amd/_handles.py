"""What the modules of the handles share: the per-device cache of library handles, the normalisation of a point-cloud
or correspondence argument and of a per-problem argument, the pointer-and-count arrays of a batched call and the
option accessors of the handles that have tuning knobs (ransac.py, fgr.py, plane.py).

One C handle is kept per device, shared by every thread of the process.  A handle is not re-entrant (its stream,
device buffers and staging memory serve one call at a time) and ctypes releases the GIL during the call, so each handle
has a lock held around every call on it; calls for different devices run concurrently."""
import atexit
import ctypes as C
import os
import threading

import numpy as np


def _current_device():
    """The calling thread's current HIP device, asked of the HIP runtime this package's library is linked against
    (already loaded: RTLD_NOLOAD never loads a second runtime).  -1 when it cannot be asked."""
    for name in ("libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"):
        try:
            rt = C.CDLL(name, mode=os.RTLD_NOLOAD | os.RTLD_GLOBAL)
        except OSError:
            continue
        d = C.c_int(-1)
        return d.value if rt.hipGetDevice(C.byref(d)) == 0 else -1
    return -1


class Handle:
    """One C handle `h` and the `lock` that serialises its calls; unpacks as (h, lock)."""

    def __init__(self, L, prefix, device):
        from . import TeaserHipError
        self._lib, self._prefix = L, prefix
        self.h = C.c_void_p()
        rc = getattr(L, prefix + "_create")(device, C.byref(self.h))
        if rc != 0:
            raise TeaserHipError(rc, "(no MI355X visible: the product has no CPU path)" if rc == 3 else "")
        self.lock = threading.Lock()

    def __iter__(self):
        return iter((self.h, self.lock))

    def call(self, fn, *args):
        """fn(h, *args) under the lock; a non-zero status raises TeaserHipError with the handle's message."""
        from . import TeaserHipError
        with self.lock:  # the handle serves one call at a time
            rc = fn(self.h, *args)
            err = getattr(self._lib, self._prefix + "_last_error")(self.h).decode() if rc != 0 else ""
        if rc != 0:
            raise TeaserHipError(rc, err)

    def close(self):
        with self.lock:
            getattr(self._lib, self._prefix + "_destroy")(self.h)


class HandleCache:
    """The handles of one kind, `prefix` naming its C functions (prefix_create, prefix_destroy, prefix_last_error);
    they are destroyed when the interpreter exits."""

    def __init__(self, prefix, handle_type=Handle):
        self.prefix, self.handle_type = prefix, handle_type
        self.handles = {}  # device ordinal -> handle
        self._handles_lock = threading.Lock()
        atexit.register(self.release)

    def get(self, device=-1):
        """The cached handle of `device`; device < 0 is resolved to the calling thread's current device first."""
        from . import lib
        L = lib()
        device = int(device)
        if device < 0:
            device = _current_device()
        with self._handles_lock:
            h = self.handles.get(device)
            if h is None:
                h = self.handles[device] = self.handle_type(L, self.prefix, device)
            return h

    def release(self):
        with self._handles_lock:
            for h in self.handles.values():
                h.close()
            self.handles.clear()


def _cloud(a, what, dtype=np.float64, kind="array"):
    """`a` as a C-contiguous n x 3 array of `dtype` (an empty one is 0 x 3); ValueError names it `what`."""
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
    if a.size == 0:
        return np.zeros((0, 3), dtype=dtype)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s must be an n x 3 %s, got shape %s" % (what, kind, a.shape))
    return a


def _pairs(corres, what):
    """`corres` as a C-contiguous n x 2 int32 array (an empty one is 0 x 2); ValueError names it `what`."""
    a = np.ascontiguousarray(np.asarray(corres, dtype=np.int32))
    if a.size == 0:
        return np.zeros((0, 2), dtype=np.int32)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("%s must be an n x 2 integer array, got shape %s" % (what, a.shape))
    return a


def _per_problem(value, b, what):
    """A per-problem argument as a list of b values: a list, tuple or array holds one per problem, anything else is
    the value of every problem."""
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != b:
            raise ValueError("%s: %d values for %d problems" % (what, len(value), b))
        return list(value)
    return [value] * b


def _rows(arrays, ptr_type):
    """What a batched C call takes for a list of 2-D arrays: the array of their row pointers (`ptr_type` each) and the
    int32 array of their row counts.  The caller keeps `arrays` and the counts alive across the call."""
    b = len(arrays)
    ptrs = (ptr_type * max(b, 1))(*[a.ctypes.data_as(ptr_type) for a in arrays])
    return ptrs, np.array([len(a) for a in arrays], dtype=np.int32)


def _set_option(cache, name, value, device):
    """prefix_set_option(name, value) on the cached handle of `device`."""
    h = cache.get(device)
    h.call(getattr(h._lib, cache.prefix + "_set_option"), name.encode(), int(value))


def _fill_scratch(cache, byte, device):
    """prefix_fill_scratch(byte) on the cached handle of `device`; the device bytes it filled."""
    h = cache.get(device)
    filled = C.c_int64()
    h.call(getattr(h._lib, cache.prefix + "_fill_scratch"), int(byte), C.byref(filled))
    return filled.value


def _get_option(cache, name, device):
    """prefix_get_option(name) on the cached handle of `device`."""
    h = cache.get(device)
    v = C.c_int64()
    h.call(getattr(h._lib, cache.prefix + "_get_option"), name.encode(), C.byref(v))
    return v.value
