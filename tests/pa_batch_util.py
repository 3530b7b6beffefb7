"""What the tests of the batched picture-analysis entries share (svt_amd_side_stats / chroma_stats / picture_detect / noise_detect _batch_launch): the return
code and the fill value they look for, a context, and device memory that is filled with SENTINEL before a batch runs."""
import ctypes as C

import numpy as np

vp = C.c_void_p
BAD_PARAM = -1                     # SVT_AMD_ERR_BAD_PARAM
SENTINEL = 0xA5                    # what the result arrays hold before a batch runs


def ok(lib, rc):
    assert rc == 0, lib.svt_amd_last_error()


def refused(lib, rc, entry, what=None):
    """the call was refused, and the error text begins with the name of the entry that was called"""
    assert rc == BAD_PARAM, (rc, what)
    assert lib.svt_amd_last_error().startswith(entry.encode() + b": "), (lib.svt_amd_last_error(), what)


def refused_as(lib, rc, text):
    """the call was refused with exactly this error text"""
    assert rc == BAD_PARAM and lib.svt_amd_last_error() == text.encode(), (rc, lib.svt_amd_last_error())


def round_up(n):
    """the next multiple of 256: where the next array of a device buffer begins"""
    return (n + 255) & ~255


def markers(lib, ctx):
    """(completion records, waits on other lanes' records) the context has issued since it was made"""
    r, w = C.c_ulonglong(), C.c_ulonglong()
    ok(lib, lib.svt_amd_debug_launch_markers(ctx, C.byref(r), C.byref(w)))
    return r.value, w.value


def make_context(lib, w, h, slots):
    ctx = vp()
    ok(lib, lib.svt_amd_context_create(0, w, h, slots, C.byref(ctx)))
    return ctx


def is_sentinel(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all())


class DeviceBuffer:
    """device memory filled with SENTINEL"""

    def __init__(self, lib, ctx, nbytes):
        self.lib, self.ctx, self.n, self.ptr = lib, ctx, nbytes, vp()
        ok(lib, lib.svt_amd_device_alloc(ctx, nbytes, C.byref(self.ptr)))
        self.fill()

    def fill(self):
        poison = np.full(self.n, SENTINEL, np.uint8)
        ok(self.lib, self.lib.svt_amd_device_upload(self.ctx, self.ptr, poison.ctypes.data, self.n))

    def at(self, offset):
        return self.ptr.value + offset

    def put(self, array, offset=0):
        """stream-ordered upload on the context's lane; the caller keeps `array` alive until the lane is synchronised"""
        ok(self.lib, self.lib.svt_amd_device_upload_async(self.ctx, vp(self.at(offset)), array.ctypes.data, array.nbytes))

    def get(self, ctx=None):
        """blocking download: waits for the stream of the context (of `ctx`, a lane, where given)"""
        out = np.zeros(self.n, np.uint8)
        ok(self.lib, self.lib.svt_amd_device_download(ctx or self.ctx, out.ctypes.data, self.ptr, self.n))
        return out

    def free(self):
        self.lib.svt_amd_device_free(self.ctx, self.ptr)
