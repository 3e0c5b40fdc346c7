"""Device copies of a C-ABI argument struct's numpy arrays, for calling a `_dev` entry point with the inputs of its host
twin (shared by the GPU tests that go through both)."""
import ctypes as C

import numpy as np


def _lib():
    import fishbirdeyevisualslam_amd as fb
    return fb.lib()


def _arrays(obj):
    """Every numpy array inside nested dicts / lists / tuples."""
    if isinstance(obj, np.ndarray):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _arrays(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _arrays(v)


class Mirror:
    """Device copies of numpy arrays, by address range: dev(p) maps a host address inside one of them to the device."""

    def __init__(self, *owners):
        import torch
        self.arrays = {a.ctypes.data: a for a in _arrays(owners)}
        self.tensors = {base: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()
                        for base, a in self.arrays.items()}

    def dev(self, p):
        for base, a in self.arrays.items():
            if base <= p < base + max(a.nbytes, 1):
                return self.tensors[base].data_ptr() + (p - base)
        raise AssertionError("pointer 0x%x is not inside any of the problem's arrays" % p)

    def struct(self, s, host_fields=()):
        """A copy of ctypes struct `s` (nested structs included) with every non-null pointer moved to the device."""
        d = type(s).from_buffer_copy(s)
        self._walk(d, host_fields)
        return d

    def _walk(self, s, host_fields):
        for name, ftype in s._fields_:
            if ftype is C.c_void_p:
                p = getattr(s, name)
                if p and name not in host_fields:
                    setattr(s, name, self.dev(p))
            elif isinstance(ftype, type) and issubclass(ftype, C.Structure):
                self._walk(getattr(s, name), host_fields)

    def host(self, arr):
        """The device copy of `arr` as a host array of the same dtype and shape."""
        return self.tensors[arr.ctypes.data].cpu().numpy().view(arr.dtype).reshape(arr.shape)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    import torch
    torch.cuda.synchronize()
