"""Spacing-aware resampling of a volume: images, label volumes and class probabilities onto another grid over the same extent.

Geometry.  A volume of logical shape (d0, d1, d2) is resampled to the shape (e0, e1, e2); the geometry always follows the two
shapes, so the physical extent is preserved (`resampled_shape` turns spacings into a shape and says which spacing the result
really has).  Per axis with n_in, n_out and the output index o, all in exact integer arithmetic:

    num = max((2 * o + 1) * n_in - n_out, 0)       den = 2 * n_out
    lo  = min(num // den, n_in - 1)                hi  = min(lo + 1, n_in - 1)
    w1  = float64(num - lo * den) / float64(den)   (one IEEE division)        w0 = 1.0 - w1

the half-pixel-centre map s = (o + 0.5) * n_in / n_out - 0.5 clamped at both ends, its fraction a single correctly rounded
quotient of two exact integers (scipy.ndimage.zoom(order=1, mode='nearest', grid_mode=True) and F.interpolate(trilinear,
align_corners=False) use the same map).  An axis with n_in == n_out has w1 == 0 exactly: per-slice (2-D) resampling is a matter
of the shapes, and an identity shape returns the input values.

Order 1.  The eight corners are visited in the order (a, b, c) = 000, 001, 010, .. 111 (axis 0 slowest), corner (a, b, c) is
the voxel (lo or hi along each axis) and weighs (w_a * w_b) * w_c in exactly this association; every accumulator starts at
+0.0, and every product and every sum is rounded to float64 on its own (no fused multiply-add).  A corner of weight 0 is
still multiplied: NaN and inf propagate as the arithmetic says (and a -0.0 comes back as +0.0, the start of its sum).
Order 0.  The voxel at min(((2 * o + 1) * n_in) // (2 * n_out), n_in - 1) per axis.

image   y = float32(sum over the corners of w * float64(x)), rounded once; order 0: the voxel itself.
labels  num_classes=C: acc[c] += w for every corner whose value is c, c in 0 .. C - 1 (a value outside belongs to no class: its
        weight is dropped); the label is the first index of the largest acc -- the arg-max of the linearly interpolated one-hot
        planes, which are never formed on the device (the host statement below sums w * 1.0 and w * 0.0, the same numbers).
        num_classes=None: the same with C = 2 on (v != 0), a 0 / 1 result.  Order 0: the nearest voxel under the same class
        rule, a value outside 0 .. C - 1 is written as 0.
probs   acc[c] = sum over the corners of w * float64(p[c]); the label is the first index of the largest acc, and float32(acc)
        the resampled probabilities.
"The largest" is found with a strict > from class 0 on: the lowest class wins a tie and a NaN never displaces an earlier class.
Why float64 accumulators: with them a float32 image result is the correctly rounded value of a sum whose own error is a few
2^-53, and class sums that are mathematically equal (eight corners of 1/8) ARE equal, so the tie rule decides and not the order
of a float32 sum.

HIP tensors take `aide_resample3d_image` / `_labels` / `_probs` (csrc/resample3d.hip: two launches, the per-axis table and one
gather), asynchronously, with nothing read on the host, and HIP tensors are returned.  numpy arrays and CPU tensors take the
numpy float64 statement in this file, which is the definition, and numpy arrays are returned.
"""
import math

import numpy as np
import torch

from ._lib import lib, check
from .ops import ptr, stream_ptr
from .volumes import MAX_VOX, classes as _classes, device_volume, host_volume, spacing as _spacing, u8

_SLAB = 1 << 21                # output voxels per pass of the host statement


def _shape3(new_shape, what):
    try:
        e = tuple(new_shape)
    except TypeError:
        e = ()
    if len(e) != 3 or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 for n in e):
        raise ValueError('%s: new_shape %r, three integers >= 0 are expected' % (what, new_shape))
    return tuple(int(n) for n in e)


def _order(order, what):
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or order not in (0, 1):
        raise ValueError('%s: order %r, 0 and 1 are supported' % (what, order))
    return int(order)


def _voxels(d, e, what, times=1):
    """the voxel counts of both sides -> True when there is nothing to compute; ValueError beyond 2^31 - 1 or for an empty input"""
    n_in, n_out = times * d[0] * d[1] * d[2], times * e[0] * e[1] * e[2]
    if max(n_in, n_out) > MAX_VOX:
        raise ValueError('%s: %d -> %d voxels, at most 2^31 - 1 on either side' % (what, n_in, n_out))
    if n_out and not n_in:
        raise ValueError('%s: an empty volume %r cannot fill new_shape %r' % (what, tuple(d), tuple(e)))
    return n_out == 0


def resampled_shape(shape, spacing, new_spacing):
    """-> ((e0, e1, e2), (s0, s1, s2)): e_k = max(1, floor(d_k * sp_k / new_k + 0.5)), the shape a volume of `shape` at `spacing`
    has at `new_spacing` (rounding half up, never below one voxel), and s_k = sp_k * d_k / e_k, the spacing the result really
    has.  ValueError for a shape that is not three integers >= 1 or spacings that are not three finite positive numbers."""
    d = _shape3(shape, 'resampled_shape')
    if min(d) < 1:
        raise ValueError('resampled_shape: shape %r, three integers >= 1 are expected' % (shape,))
    sp, new = _spacing(spacing, 'resampled_shape'), _spacing(new_spacing, 'resampled_shape')
    e = tuple(max(1, int(math.floor(n * s / t + 0.5))) for n, s, t in zip(d, sp, new))
    return e, tuple(s * n / m for n, s, m in zip(d, sp, e))


# ---- the host statement ----------------------------------------------------------------------------------------------------
def axis_table(n_in, n_out):
    """-> (lo, hi, w1) of every output index of one axis: int64, int64, float64"""
    o = np.arange(n_out, dtype=np.int64)
    den = 2 * n_out
    num = np.maximum((2 * o + 1) * n_in - n_out, 0)
    lo = np.minimum(num // max(den, 1), n_in - 1)
    hi = np.minimum(lo + 1, n_in - 1)
    return lo, hi, (num - lo * den).astype(np.float64) / np.float64(max(den, 1))


def nearest_table(n_in, n_out):
    o = np.arange(n_out, dtype=np.int64)
    return np.minimum(((2 * o + 1) * n_in) // max(2 * n_out, 1), n_in - 1)


def _first_max(acc):
    """[C, ...] -> int64 [...]: the first index of the largest value, by a strict > from index 0 on"""
    best, top = np.zeros(acc.shape[1:], np.int64), acc[0].copy()
    for c in range(1, acc.shape[0]):
        m = acc[c] > top
        best[m] = c
        top[m] = acc[c][m]
    return best


def _interp(x, e):
    """float64 [..., d0, d1, d2] -> the float64 accumulators [..., e0, e1, e2] of order 1"""
    d = x.shape[-3:]
    tabs = [axis_table(n, m) for n, m in zip(d, e)]
    out = np.empty(x.shape[:-3] + tuple(e), np.float64)
    lead = int(np.prod(x.shape[:-3], dtype=np.int64))
    step = max(1, _SLAB // max(1, lead * e[1] * e[2]))
    for start in range(0, e[0], step):
        sl = slice(start, start + step)
        acc = np.zeros(out[..., sl, :, :].shape, np.float64)
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    (i0, w0), (i1, w1), (i2, w2) = ((t[k], t[2] if k else 1.0 - t[2]) for t, k in zip(tabs, (a, b, c)))
                    w = (w0[sl, None, None] * w1[None, :, None]) * w2[None, None, :]
                    acc = acc + w * x[(Ellipsis,) + np.ix_(i0[sl], i1, i2)]
        out[..., sl, :, :] = acc
    return out


def _nearest(x, e):
    return x[(Ellipsis,) + np.ix_(*(nearest_table(n, m) for n, m in zip(x.shape[-3:], e)))]


def _labels_host(vol, e, c, order):
    cls = (vol != 0).astype(np.int64) if c is None else vol.astype(np.int64)
    c = c or 2
    if order == 0:
        v = _nearest(cls, e)
        return np.where((v >= 0) & (v < c), v, 0).astype(np.uint8)
    onehot = (cls[None] == np.arange(c, dtype=np.int64)[:, None, None, None]).astype(np.float64)
    return _first_max(_interp(onehot, e)).astype(np.uint8)


# ---- the operators ---------------------------------------------------------------------------------------------------------
def _workspace(e, device):
    return torch.empty(lib.aide_resample3d_ws_bytes(*e), device=device, dtype=torch.uint8)


def resample_image(x, new_shape, order=1):
    """float32 [..., d0, d1, d2] -> float32 [..., e0, e1, e2]; the leading dims are a batch.  order 1: trilinear with float64
    accumulators, rounded once; order 0: the nearest voxel.  RuntimeError for fewer than three dims or another dtype,
    ValueError for order, new_shape, more than 2^31 - 1 voxels on either side (the batch counts) or an empty input."""
    e, order = _shape3(new_shape, 'resample_image'), _order(order, 'resample_image')
    dev = isinstance(x, torch.Tensor) and x.is_cuda
    if not dev:
        x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if len(x.shape) < 3:
        raise RuntimeError('resample_image: [..., d0, d1, d2] expected, got %d dims' % len(x.shape))
    if x.dtype != (torch.float32 if dev else np.float32):
        raise RuntimeError('resample_image: float32 expected, got %s' % x.dtype)
    lead, d = tuple(x.shape[:-3]), tuple(x.shape[-3:])
    batch = int(np.prod(lead, dtype=np.int64))
    empty = _voxels(d, e, 'resample_image', batch)
    if not dev:
        if empty:
            return np.zeros(lead + e, np.float32)
        return np.ascontiguousarray(_nearest(x, e)) if order == 0 else _interp(x.astype(np.float64), e).astype(np.float32)
    out = torch.empty(lead + e, device=x.device, dtype=torch.float32)
    if empty:
        return out
    xb = x.detach().reshape((batch,) + d)
    check(lib.aide_resample3d_image(ptr(xb), batch, xb.stride(0), *d, *xb.stride()[1:], *e, order, ptr(out),
                                    ptr(_workspace(e, x.device)), stream_ptr()), 'resample3d_image')
    return out


def resample_labels(volume, new_shape, num_classes=None, order=1):
    """An integer volume [d0, d1, d2] -> uint8 [e0, e1, e2].  num_classes=C (2 .. 8): the first class of the largest
    interpolated indicator (order 1) or the nearest voxel (order 0), a value outside 0 .. C - 1 belonging to no class;
    num_classes=None: the 0 / 1 result of C = 2 on (volume != 0).  A HIP result is dense in the memory order of the volume (a
    permuted view stays one: loads and stores both coalesce); its values do not depend on the strides.  RuntimeError for dims
    or dtype, ValueError for num_classes, order, new_shape, more than 2^31 - 1 voxels on either side or an empty input."""
    what = 'resample_labels'
    e, c, order = _shape3(new_shape, what), _classes(num_classes, what), _order(order, what)
    if not (isinstance(volume, torch.Tensor) and volume.is_cuda):
        vol = host_volume(volume, what)
        return np.zeros(e, np.uint8) if _voxels(vol.shape, e, what) else _labels_host(vol, e, c, order)
    if volume.dim() == 3:
        empty = _voxels(volume.shape, e, what)
    v = device_volume(volume, what, keep_uint8=True)
    oa = sorted(range(3), key=lambda k: (-v.stride(k), k))        # the logical axes from the slowest to the fastest in memory
    strides, run = [0, 0, 0], 1
    for k in reversed(oa):
        strides[k], run = run, run * max(e[k], 1)
    out = torch.empty_strided(e, strides, device=v.device, dtype=torch.uint8)
    if empty:
        return out
    check(lib.aide_resample3d_labels(ptr(v), u8(v), *v.shape, *v.stride(), *e, c or 0, order, *oa, ptr(out),
                                     ptr(_workspace(e, v.device)), stream_ptr()), 'resample3d_labels')
    return out


def resample_probs(probs, new_shape, probs_out=False):
    """float32 probabilities [S, C, H, W] (C = 2 .. 8; any strides, taken without a copy) resampled over the axes (S, H, W) to
    new_shape = (S', H', W') -> labels int64 [S', H', W'], the first class of the largest interpolated probability; with
    probs_out=True (labels, float32 [S', C, H', W']).  RuntimeError for dims, C or dtype, ValueError for new_shape, more than
    2^31 - 1 voxels on either side (the classes count) or an empty input."""
    what = 'resample_probs'
    e = _shape3(new_shape, what)
    dev = isinstance(probs, torch.Tensor) and probs.is_cuda
    if not dev:
        probs = probs.detach().cpu().numpy() if isinstance(probs, torch.Tensor) else np.asarray(probs)
    if len(probs.shape) != 4 or not 2 <= probs.shape[1] <= 8 or probs.dtype != (torch.float32 if dev else np.float32):
        raise RuntimeError('%s: float32 [S,C,H,W] with 2 <= C <= 8 expected, got %s %r' % (what, probs.dtype, tuple(probs.shape)))
    s, c, h, w = probs.shape
    empty = _voxels((s, h, w), e, what, c)
    if not dev:
        if empty:
            labels, acc = np.zeros(e, np.int64), np.zeros((c,) + e, np.float64)
        else:
            acc = _interp(probs.transpose(1, 0, 2, 3).astype(np.float64), e)
            labels = _first_max(acc)
        return (labels, np.ascontiguousarray(acc.astype(np.float32).transpose(1, 0, 2, 3))) if probs_out else labels
    p = probs.detach()
    labels = torch.empty(e, device=p.device, dtype=torch.int64)
    out = torch.empty((e[0], c, e[1], e[2]), device=p.device, dtype=torch.float32) if probs_out else None
    if not empty:
        check(lib.aide_resample3d_probs(ptr(p), c, p.stride(1), s, h, w, p.stride(0), p.stride(2), p.stride(3), *e, ptr(labels),
                                        ptr(out), ptr(_workspace(e, p.device)), stream_ptr()),
              'resample3d_probs')
    return (labels, out) if probs_out else labels
