"""What the Python side of every 3-D volume operator shares (postprocess.py, inference.py, morphology.py, utils/metrics3d.py):
the checks of a label volume and of num_classes / spacing, and the marshalling of a strided HIP volume for the C entry points,
which read int64 or uint8 voxels through element strides and address them with 32-bit indices."""
import math

import numpy as np
import torch

INT_DTYPES = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool)
MAX_VOX = 2 ** 31 - 1


def _integer_below_limit(x, what):
    if x.dtype not in INT_DTYPES:
        raise RuntimeError('%s: integer labels expected, got %s' % (what, x.dtype))
    if x.numel() > MAX_VOX:
        raise RuntimeError('%s: %d voxels, at most 2^31 - 1' % (what, x.numel()))


def widen(x, keep_uint8=False):
    """detached and int64 (uint8 stays with keep_uint8), the strides untouched"""
    x = x.detach()
    return x if x.dtype == torch.int64 or (keep_uint8 and x.dtype == torch.uint8) else x.to(torch.int64)


def volume_args(x, what):
    """The argument checks of a device operator (before anything is launched): a 3-D integer tensor of < 2^31 voxels,
    RuntimeError otherwise."""
    if x.dim() != 3:
        raise RuntimeError('%s: a 3-D volume is expected, got %d dims' % (what, x.dim()))
    _integer_below_limit(x, what)


def device_volume(x, what, keep_uint8=False):
    """`volume_args`, then `widen`: what a C entry point reads"""
    volume_args(x, what)
    return widen(x, keep_uint8)


def as3d(x):
    """detached, int64 or uint8, exactly three dims: leading dims of 1 are added, more than three are flattened into the first"""
    x = widen(x, True)
    if x.dim() > 3:
        x = x.reshape((-1,) + tuple(x.shape[-2:]))
    while x.dim() < 3:
        x = x.unsqueeze(0)
    return x


def device_pair(pred, target, what):
    """The checks of the device scores: integer volumes of the same shape, at least one dim, < 2^31 voxels -> both `as3d`"""
    if tuple(pred.shape) != tuple(target.shape):
        raise RuntimeError('%s: shape mismatch %s vs %s' % (what, tuple(pred.shape), tuple(target.shape)))
    if pred.dim() == 0:
        raise RuntimeError('%s: volumes of at least one dim expected' % what)
    for x in (pred, target):
        _integer_below_limit(x, what)
    return as3d(pred), as3d(target)


def host_volume(x, what):
    """numpy array or tensor -> a 3-D integer (or bool) numpy array, RuntimeError otherwise"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.ndim != 3:
        raise RuntimeError('%s: a 3-D volume is expected, got %d dims' % (what, x.ndim))
    if x.dtype != np.bool_ and not np.issubdtype(x.dtype, np.integer):
        raise RuntimeError('%s: integer labels expected, got %s' % (what, x.dtype))
    return x


def classes(num_classes, what, strict=True):
    """num_classes -> None or an int in 2 .. 8.  strict: None or a true integer, ValueError otherwise.  strict=False, the rule of
    the older entry points: whatever int() takes (None is the caller's business), RuntimeError outside 2 .. 8."""
    if not strict:
        c = int(num_classes)
        if not 2 <= c <= 8:
            raise RuntimeError('%s: num_classes %d, 2 .. 8 are supported' % (what, c))
        return c
    if num_classes is None:
        return None
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 2 <= num_classes <= 8:
        raise ValueError('%s: num_classes %r, None or 2 .. 8 are supported' % (what, num_classes))
    return int(num_classes)


def spacing(spacing, what):
    """-> (sp0, sp1, sp2) as floats: three finite positive numbers, ValueError otherwise"""
    try:
        sp = tuple(float(s) for s in spacing)
    except TypeError:
        sp = ()
    if len(sp) != 3 or not all(math.isfinite(s) and s > 0.0 for s in sp):
        raise ValueError('%s: spacing %r, three finite positive numbers are expected' % (what, spacing))
    return sp


def u8(x):
    """the element-type flag of the C entry points"""
    return int(x.dtype == torch.uint8)


def workspace(ws_bytes, like, *args):
    """the workspace of an operator for the voxels of `like`: ws_bytes = its *_ws_bytes entry, args what that takes after nvox"""
    return torch.empty(ws_bytes(like.numel(), *args), device=like.device, dtype=torch.uint8)
