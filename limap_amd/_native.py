"""The one way from a caller's NumPy array or torch tensor to a pointer in a native struct.

Two rules live here and nowhere else.  The device rule: a GPU tensor is read in place only where it lives on the device
the call runs on (`check_device`, which `operand` applies).  The stream rule: `wait_for_torch`.  This module imports
neither torch nor the library when it is imported."""
import numpy as np


def is_torch(x):
    return type(x).__module__.startswith("torch")


def to_host(x):
    return x.detach().cpu().numpy() if is_torch(x) else np.asarray(x)


def address(a):
    return a.data_ptr() if is_torch(a) else a.ctypes.data


def check_device(x, *, host, device, who, what):
    """1 where the call reads x in place on the device, 0 where it takes a host array: a GPU tensor stays where it is
    unless the host path was asked for, and then it must live on `device`, the device of the call's context (None
    where a converter runs before that context is known: its caller asks again, with the device, before the call)"""
    if host or not (is_torch(x) and x.is_cuda):
        return 0
    if device is not None and x.device.index != device:
        raise ValueError(f"{who}: {what} lives on {x.device}, the call runs on cuda:{device}")
    return 1


class Operand:
    """One view of "NumPy array or torch tensor": `keep` owns the memory behind `address`, `on_device` says where that
    is.  Shape, dtype (a NumPy-style name) and strides (in elements) are read without converting anything; `astype` and
    `contiguous` give a new Operand and copy only where they must.  What NumPy and torch spell alike (`.T`, `reshape`,
    an index) a converter applies through `map`."""

    def __init__(self, keep, on_device=0):
        self.keep, self.on_device = keep, on_device

    shape = property(lambda self: tuple(int(v) for v in self.keep.shape))
    ndim = property(lambda self: len(self.keep.shape))
    dtype = property(lambda self: str(self.keep.dtype).split(".")[-1])
    address = property(lambda self: address(self.keep))

    @property
    def strides(self):
        k = self.keep
        return tuple(k.stride()) if is_torch(k) else tuple(s // k.itemsize for s in k.strides)

    def map(self, fn):
        """the Operand of fn(keep) in the same place"""
        keep = fn(self.keep)
        return self if keep is self.keep else Operand(keep, self.on_device)

    def astype(self, name):
        if self.dtype == name:
            return self
        if is_torch(self.keep):
            import torch
            keep = self.keep.to(getattr(torch, name))  # (a host Operand ends as an array: only bfloat16 waits here)
            return Operand(keep if self.on_device else keep.numpy(), self.on_device)
        return self.map(lambda k: k.astype(name))

    def contiguous(self):
        return self.map(lambda k: k.contiguous() if is_torch(k) else np.ascontiguousarray(k))


def operand(x, *, host, device, who, what):
    """The Operand of an input of a native call on `device`: a GPU tensor on that device stays a tensor (on_device 1)
    unless `host`; one on another device is refused; everything else becomes a host array whose strides are whole
    elements (a CPU tensor shares its memory; bfloat16, which NumPy lacks, stays a CPU tensor until `astype` makes an
    array of it, so that a tensor in `keep` with on_device 0 is bfloat16 and nothing else)."""
    if check_device(x, host=host, device=device, who=who, what=what):
        return Operand(x, 1)
    if is_torch(x) and str(x.dtype) == "torch.bfloat16":
        return Operand(x.detach().cpu())
    a = to_host(x)
    if any(s % a.itemsize for s in a.strides) or not a.flags.aligned:
        a = np.ascontiguousarray(a)
    return Operand(a)


def wait_for_torch(device):
    """The context's stream does not wait for torch's streams: whatever torch has enqueued on `device` -- a tensor a
    network has just written, a conversion of `Operand`, an output allocated for the call -- must be finished before a
    native call reads or writes it in place.  Once per such call, directly before it."""
    import torch
    torch.cuda.synchronize(device)


def raise_host_error(L, getter, prefix=""):
    """the refusal of a host-only entry point (`lt_fn_*`), from the error slot `getter` names"""
    raise ValueError(prefix + getattr(L, getter)().decode(errors="replace"))


def csr(parts, width):
    """per-image (n_i, width) float64 arrays -> (offsets (len + 1,) int64, one contiguous array; a zero row if empty)"""
    off = np.zeros(len(parts) + 1, np.int64)
    for k, a in enumerate(parts):
        off[k + 1] = off[k] + a.shape[0]
    flat = np.ascontiguousarray(np.concatenate(parts, 0), np.float64) if off[-1] else np.zeros((1, width))
    return off, flat


def host_threads(host, host_threads):
    """the thread count that selects a module's host path (None: the device path)"""
    return host_threads if host_threads is not None else (0 if host else None)
