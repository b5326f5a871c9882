"""Ball morphology in millimetres and the Euclidean distance transform of a label volume.

Spacing.  spacing = (sp0, sp1, sp2), finite and > 0, the edge lengths of a voxel in the order of the volume's axes.

Squared length of an integer offset o, in float64 and in exactly this association (the order in which the separable passes
of the kernels along d2, d1 and d0 accumulate; host and device use the same expression, so a tie q == r * r falls the same way
wherever the arithmetic is exact):

    q(o) = (sp0 * o0)**2 + ((sp1 * o1)**2 + (sp2 * o2)**2)

Ball.  B(r) = {o : q(o) <= r * r}, r finite and >= 0; B(0) = {0}.  An axis with sp_k > r contributes only offset 0: per-slice
(2-D disk) morphology is a matter of the spacing passed.

Foreground X: v != 0, or v == c for a class c.
dilate(X, r)(v)          = some u in X inside the volume has (v - u) in B(r)        scipy binary_dilation(X, structure=B)
erode(X, r, outside)(v)  = X~(v + o) for every o in B(r), X~ = X inside the volume and the constant `outside` beyond it
                                                                      scipy binary_erosion(X, structure=B, border_value=outside)
open_(X, r)  = dilate(erode(X, r, 0), r)    anti-extensive
close(X, r)  = erode(dilate(X, r), r, 1)    extensive: the outside counts as foreground, or objects on a face would be eaten
distance_transform(X)(v) = 0 on the background, sqrt(min over background u of q(v - u)) on the foreground
                           (scipy distance_transform_edt(X, sampling=spacing)); +inf everywhere without a background voxel

Classes (num_classes=C, 2 .. 8): every plane X_c = (v == c), c = 1 .. C - 1, is transformed on its own.  erode / open_: the
result is c where plane c survives, 0 elsewhere.  dilate / close: a voxel whose value is in 1 .. C - 1 keeps it (a class never
overwrites another), any other voxel becomes c if exactly one class claims it and stays 0 if several do (the rule of
`fill_holes`: mixed is not guessed at).  Values outside 0 .. C - 1 belong to no class and are written as 0.
num_classes=None: X = (v != 0), the result is 0 / 1; C = 2 on a {0, 1} volume gives the same bytes.

HIP tensors (int64 or uint8, other integer types are widened; any strides) take `aide_morph3d` / `aide_edt3d`
(csrc/morph3d.hip, csrc/surface3d.hip), asynchronously, and HIP tensors are returned.  numpy arrays and CPU tensors take scipy,
which is the definition, and numpy arrays are returned.
"""
import ctypes
import math

import numpy as np
import torch

from ._lib import lib, check
from .ops import ptr, stream_ptr
from .volumes import classes as _classes, device_volume, host_volume, spacing as _spacing, u8, workspace

OPS = {'erode0': 0, 'erode1': 1, 'dilate': 2, 'open': 3, 'close': 4}


def _radius(radius, what):
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) \
            or not math.isfinite(radius) or radius < 0:
        raise ValueError('%s: radius %r, a finite number >= 0 is expected' % (what, radius))
    return float(radius)


def _window(r, sp, limit=None):
    """the largest w (<= limit) with (sp * w)**2 <= r * r"""
    r2 = r * r
    w = int(min(math.floor(r / sp), 2 ** 40 if limit is None else limit))
    while (limit is None or w < limit) and (sp * (w + 1)) * (sp * (w + 1)) <= r2:
        w += 1
    while w > 0 and (sp * w) * (sp * w) > r2:
        w -= 1
    return w


def _ball(r, sp, limits=(None, None, None)):
    w = [_window(r, s, m) for s, m in zip(sp, limits)]
    o0, o1, o2 = np.ogrid[-w[0]:w[0] + 1, -w[1]:w[1] + 1, -w[2]:w[2] + 1]
    t0, t1, t2 = (s * o.astype(np.float64) for s, o in zip(sp, (o0, o1, o2)))
    return t0 * t0 + (t1 * t1 + t2 * t2) <= r * r


def ball(radius, spacing=(1.0, 1.0, 1.0)):
    """The structuring element B(radius): a boolean array of shape (2 W0 + 1, 2 W1 + 1, 2 W2 + 1), W_k = floor(radius / sp_k),
    centred on offset 0, True where q(o) <= radius * radius."""
    return _ball(_radius(radius, 'ball'), _spacing(spacing, 'ball'))


def _plane_host(x, op, b):
    """one boolean plane through scipy"""
    from scipy import ndimage
    if op == 'erode0':
        return ndimage.binary_erosion(x, structure=b, border_value=0)
    if op == 'erode1':
        return ndimage.binary_erosion(x, structure=b, border_value=1)
    if op == 'dilate':
        return ndimage.binary_dilation(x, structure=b)
    if op == 'open':
        return ndimage.binary_dilation(ndimage.binary_erosion(x, structure=b, border_value=0), structure=b)
    return ndimage.binary_erosion(ndimage.binary_dilation(x, structure=b), structure=b, border_value=1)


def _morph_host(vol, op, r, sp, c):
    """the host statement of aide_morph3d"""
    cmap = (vol != 0).astype(np.uint8) if c is None else np.where((vol >= 1) & (vol < c), vol, 0).astype(np.uint8)
    if vol.size == 0:
        return cmap
    b = _ball(r, sp, vol.shape)                   # offsets beyond the volume's extent can reach nothing, not even its outside
    planes = [(k, _plane_host(cmap == k, op, b)) for k in range(1, c or 2)]
    if op in ('erode0', 'erode1', 'open'):
        out = np.zeros(vol.shape, np.uint8)
        for k, p in planes:
            out[p] = k
        return out
    claims = np.zeros(vol.shape, np.int64)
    which = np.zeros(vol.shape, np.uint8)
    for k, p in planes:
        claims += p
        which[p] = k
    return np.where(cmap != 0, cmap, np.where(claims == 1, which, 0)).astype(np.uint8)


def _morph(volume, op, radius, spacing, num_classes, what):
    r, sp, c = _radius(radius, what), _spacing(spacing, what), _classes(num_classes, what)
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        v = device_volume(volume, what, keep_uint8=True)
        out = torch.empty(v.shape, device=v.device, dtype=torch.uint8)
        if v.numel() == 0:
            return out
        ws = workspace(lib.aide_morph3d_ws_bytes, v)
        check(lib.aide_morph3d(ptr(v), u8(v), *v.shape, *v.stride(), c or 0, OPS[op], r,
                               (ctypes.c_double * 3)(*sp), ptr(out), ptr(ws), stream_ptr()), 'morph3d')
        return out
    return _morph_host(host_volume(volume, what), op, r, sp, c)


def erode(volume, radius, spacing=(1.0, 1.0, 1.0), num_classes=None, outside=0):
    """Erosion with the ball B(radius) in the units of `spacing`; outside = 0 or 1: what lies beyond the volume (0: a voxel
    within `radius` of a face of the volume is eroded).  uint8 of the volume's shape.  ValueError for a radius that is negative
    or not finite, a spacing that is not three finite positive numbers, num_classes other than None or 2 .. 8, another outside."""
    if isinstance(outside, bool) or outside not in (0, 1):
        raise ValueError('erode: outside %r, 0 or 1 are supported' % (outside,))
    return _morph(volume, 'erode1' if outside else 'erode0', radius, spacing, num_classes, 'erode')


def dilate(volume, radius, spacing=(1.0, 1.0, 1.0), num_classes=None):
    """Dilation with the ball B(radius); with num_classes a class never overwrites another and a voxel that several classes
    claim stays 0.  Arguments and errors as for `erode`."""
    return _morph(volume, 'dilate', radius, spacing, num_classes, 'dilate')


def open_(volume, radius, spacing=(1.0, 1.0, 1.0), num_classes=None):
    """Opening dilate(erode(X, radius, 0), radius): removes what the ball does not fit into (speckle, thin bridges) and never
    adds a voxel.  Arguments and errors as for `erode`."""
    return _morph(volume, 'open', radius, spacing, num_classes, 'open_')


def close(volume, radius, spacing=(1.0, 1.0, 1.0), num_classes=None):
    """Closing erode(dilate(X, radius), radius, 1): seals gaps narrower than the ball and never removes a voxel.  Arguments and
    errors as for `erode`."""
    return _morph(volume, 'close', radius, spacing, num_classes, 'close')


def distance_transform(volume, spacing=(1.0, 1.0, 1.0), cls=None):
    """float64 [d0,d1,d2], contiguous: 0 on the background, on the foreground (volume != 0, or volume == cls) the Euclidean
    distance in the units of `spacing` to the nearest background voxel; +inf everywhere when there is no background voxel.
    HIP tensor: `aide_edt3d`, four launches; otherwise scipy.ndimage.distance_transform_edt(fg, sampling=spacing)."""
    sp = _spacing(spacing, 'distance_transform')
    if cls is not None and (isinstance(cls, bool) or not isinstance(cls, (int, np.integer)) or not 0 <= cls < 2 ** 31):
        raise ValueError('distance_transform: cls %r, None or a class value >= 0 is expected' % (cls,))
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        v = device_volume(volume, 'distance_transform', keep_uint8=True)
        dist = torch.empty(v.shape, device=v.device, dtype=torch.float64)
        if v.numel() == 0:
            return dist
        ws = workspace(lib.aide_edt3d_ws_bytes, v)
        check(lib.aide_edt3d(ptr(v), u8(v), *v.shape, *v.stride(), -1 if cls is None else int(cls),
                             (ctypes.c_double * 3)(*sp), ptr(dist), ptr(ws), stream_ptr()), 'edt3d')
        return dist
    vol = host_volume(volume, 'distance_transform')
    fg = (vol != 0) if cls is None else (vol == cls)
    if fg.size == 0:
        return np.zeros(fg.shape, np.float64)
    if fg.all():                                  # scipy's result is undefined without a background voxel
        return np.full(fg.shape, np.inf, np.float64)
    from scipy import ndimage
    return np.ascontiguousarray(ndimage.distance_transform_edt(fg, sampling=sp), dtype=np.float64)
