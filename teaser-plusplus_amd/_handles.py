"""What icp.py, voxel.py and features.py share: the per-device cache of library handles and the normalisation of a
point-cloud argument.

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
