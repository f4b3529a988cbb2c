"""What the fused classes share: a handle of the HIP library bound to one GPU (``Handle``: creation, the error message of a
failed call, stream rebinding, teardown, input coercion) and the flat gradient buffer of the two ``backward`` classes
(``GradBuffer``)."""
from __future__ import annotations

import ctypes as C

from . import _capi


class Handle:
    """One ``<PREFIX>_create``d object of the library on one GPU.  Every launch goes to torch's current stream of that
    device: a method calls ``_bind_stream()`` before its launch and ``_check(rc, what)`` after it."""
    PREFIX = ""                # the family's C prefix: <PREFIX>_create / _destroy / _set_stream / _last_error
    LAST_ERROR = None          # the function that holds the message of a failed create; None: the family's own
    HAS_LAST_ERROR = True      # False: the family has no <PREFIX>_last_error, a failed call reports its code alone
    _h = None                  # (so that close() is safe on an object whose __init__ raised)

    def __init__(self, device: int, *create_args, check_device=None):
        """create_args: what ``<PREFIX>_create`` takes between the stream and the out pointer.  check_device(torch.device):
        the spec's refusal of tensors that live elsewhere, made before anything is created."""
        import torch
        self._torch = torch
        self._L = L = _capi.load()
        name = type(self).__name__
        if not torch.cuda.is_available():
            raise _capi.MeshEnvError(f"{name} needs a ROCm GPU")
        self.device = torch.device("cuda", device)
        if check_device is not None:
            check_device(self.device)
        self._h = C.c_void_p()
        self._set_stream = getattr(L, self.PREFIX + "_set_stream")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = getattr(L, self.PREFIX + "_create")(device, C.c_void_p(stream), *create_args, C.byref(self._h))
        if rc != 0:
            msg = getattr(L, self.LAST_ERROR or self.PREFIX + "_last_error")(None)
            raise _capi.MeshEnvError(f"{self.PREFIX}_create failed ({rc}): {msg.decode() if msg else ''}")
        self._stream = stream

    def _check(self, rc, what):
        if rc != 0:
            msg = getattr(self._L, self.PREFIX + "_last_error")(self._h) if self.HAS_LAST_ERROR else None
            raise _capi.MeshEnvError(f"{what} failed (code {rc})" + (f": {msg.decode()}" if msg is not None else ""))

    def _bind_stream(self):
        stream = self._torch.cuda.current_stream(self.device).cuda_stream
        if stream != self._stream:
            self._check(self._set_stream(self._h, C.c_void_p(stream)), self.PREFIX + "_set_stream")
            self._stream = stream

    def _f32(self, x, name, shape):
        """x as a float32 contiguous tensor on the handle's device, detached, of one of the shapes in `shape`."""
        t = self._torch
        if x.requires_grad:
            x = x.detach()
        if x.dtype != t.float32 or not x.is_contiguous() or x.device != self.device:
            x = x.to(device=self.device, dtype=t.float32).contiguous()
        if tuple(x.shape) not in shape:
            raise ValueError(f"{name} must have shape {' or '.join(str(s) for s in shape)}, got {tuple(x.shape)}")
        return x

    @staticmethod
    def _ptrs(tensors):
        """A C array of the tensors' device pointers (a ``const float *const *`` argument)."""
        return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def close(self):
        if self._h:
            getattr(self._L, self.PREFIX + "_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GradBuffer:
    """The flat gradient buffer of a Handle whose ``spec`` lays it out (``n_grad`` floats, ``offsets()``): the kernels write
    it, and ``p.grad`` of every parameter is a view into it."""

    def _alloc_grads(self):
        self.grad_buffer = self._torch.zeros(self.spec.n_grad, dtype=self._torch.float32, device=self.device)
        self._views = []

    def _view_grads(self):
        """After a bind: one view per parameter, in the spec's order."""
        self._views = [(p, self.grad_buffer[at:at + p.numel()].view(p.shape)) for p, at in self.spec.offsets()]

    def _attach(self):
        """p.grad of every parameter is its view of the gradient buffer: whatever it held (None, a tensor of the caller's)
        is replaced; host-side pointer comparisons only."""
        for p, v in self._views:
            g = p.grad
            if g is None or g.data_ptr() != v.data_ptr() or g.shape != v.shape or g.dtype != v.dtype or not g.is_contiguous():
                p.grad = v
