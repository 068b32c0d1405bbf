"""What the wrappers of the three layer kernels share (gru.py, mlp.py, gnn.py): what a float32 device argument is, how backward's workspace is chosen
and how a plan reaches its C entry. The C half of the same decisions is csrc/gmpe_host.h."""
import ctypes as C

import torch

from . import _lib
from .engine import _ordinal, _stream_of, _workspace


def tensor_attr(obj, path, attr, why=""):
    """obj.attr, a tensor; `path` names obj in the complaint"""
    t = getattr(obj, attr, None)
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s.%s is missing or no tensor%s" % (path, attr, why))
    return t


def need_float32(fn, tensors):
    """every (name, tensor) is float32; half precision is refused by the name of the public function `fn`"""
    for name, t in tensors:
        if t.dtype in (torch.float16, torch.bfloat16):
            raise NotImplementedError("%s is %s: %s is float32 only (half precision is not supported)" % (name, t.dtype, fn))
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, not %s" % (name, t.dtype))


def need_device(tensors, dev, anchor):
    """every (name, tensor) is on `dev`, the device of the argument called `anchor`"""
    for name, t in tensors:
        if t.device != dev:
            raise ValueError("%s must be on %s (the device of %s)" % (name, dev, anchor))


def backward_workspace(train, nbytes, workspace, dev):
    """The workspace of a training call — the caller's, checked against nbytes(), or a fresh one — or None for a forward-only call, whose caller's
    workspace is checked for what it is and left alone. nbytes is asked only when training."""
    if train:
        return _workspace(nbytes(), workspace, dev)
    if workspace is not None:
        _workspace(0, workspace, dev)
    return None


def run(entry, dev, plan):
    """the C entry `entry`(device, plan, stream) on dev's current stream"""
    _lib.check(getattr(_lib.load(), entry)(_ordinal(dev), C.byref(plan), _stream_of(dev)), entry)
