"""Sliding-window inference: overlapping windows of the training size over an image of any size, and the weighted blend of
their soft-max maps (what nnU-Net and MONAI's `sliding_window_inference` do), on the native grid of the image.

Grid.  Along an axis of length `size`, with window `win` and stride `s` (1 <= s <= win): starts = [0] when size <= win,
otherwise [0, s, 2 s, ... (every k s < size - win)] + [size - win]: the last window is clamped to end at the border, no start
lies outside the image, every pixel is covered.  Windows are numbered in raster order b = a_y * len(starts_x) + a_x; at most
32 starts per axis (ValueError beyond).

Stack.  y[b][n][c][u][v] = x[n][c][min(sy_b + u, H - 1)][min(sx_b + v, W - 1)], shape [B,N,C,wh,ww]: plane b is window b of
every image (the layout of `view_stack`'s [V,N,...]).  Clamping is the only padding and occurs only where the image is
smaller than the window.

Weights.  w(u, v) = fp32(g_h[u]) * fp32(g_w[v]), one fp32 product.  'uniform': ones.  'gaussian': g[i] = exp(-0.5 * ((i -
(win - 1) / 2) / (sigma_scale * win))^2), computed in float64 and rounded once to fp32; sigma_scale = 0.125 by default, the
smallest corner weight is then about 1e-7, a normal fp32 number: no clamping of the weights (a sigma_scale below about
0.054, whose corner weight would underflow, raises ValueError).

Blend.  For an output pixel the windows that contain it are visited in increasing b, in fp32 and never contracted:
acc_c = acc_c + w * p_c; den = den + w, with p the fp32 soft-max of the window's logits (the operation order of
`ensemble_vote_host`) or the input itself when the caller passes probabilities.  labels = the FIRST class of the largest
acc_c (int64); probs_c = acc_c / den (fp32 [N,C,H,W], on request).  Window pixels beyond the image (the clamped padding) are
never read back.  `aide_window_stack` / `aide_window_blend` (csrc/window.hip) are one launch each, without atomics or
scratch tensors, so the output bytes repeat from call to call; `window_blend_host` is the same order of fp32 operations in
torch.
"""
import ctypes
import functools

import torch

from ._lib import lib, check
from .ops import ptr, stream_ptr
from .ensemble import MAX_CLASSES, view_codes, ensemble_vote, member_logits, _net_list, _member_count

MAX_STARTS = 32
WEIGHT_MODES = ('gaussian', 'uniform')


def _pair(value, name):
    """an int or a pair of ints -> (a, b), both positive"""
    pair = tuple(value) if isinstance(value, (tuple, list)) else (value, value)
    if len(pair) != 2 or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in pair):
        raise ValueError('%s: a positive int or a pair of them expected, got %r' % (name, value))
    return pair


def _axis_starts(size, win, stride):
    if stride > win:
        raise ValueError('window_grid: stride %d above the window %d leaves pixels uncovered' % (stride, win))
    starts = [0] if size <= win else list(range(0, size - win, stride)) + [size - win]
    if len(starts) > MAX_STARTS:
        raise ValueError('window_grid: %d window starts along an axis of %d, at most %d' % (len(starts), size, MAX_STARTS))
    return tuple(starts)


def window_grid(h, w, window, stride=None):
    """-> (starts_y, starts_x), tuples of ints, for an h x w image.  window: an int or (wh, ww); stride: an int or a pair, None:
    window // 2 per axis.  ValueError for non-positive values, a stride above the window or more than 32 starts on an axis."""
    h, w = _pair((h, w), 'window_grid: image size')
    wh, ww = _pair(window, 'window')
    sh, sw = (max(1, wh // 2), max(1, ww // 2)) if stride is None else _pair(stride, 'stride')
    return _axis_starts(h, wh, sh), _axis_starts(w, ww, sw)


def window_weights(window, weights='gaussian', sigma_scale=0.125):
    """-> (g_h [wh], g_w [ww]): the axis weights as fp32 CPU vectors; the weight of window pixel (u, v) is g_h[u] * g_w[v].
    ValueError for an unknown mode and for a sigma_scale that is not positive or so small (below about 0.054) that the corner
    weight g_h[0] * g_w[0] = exp(-0.25 / sigma_scale^2) is no normal fp32 number: a corner of the image is covered by one
    window only, and a weight of 0 there would leave 0 / 0."""
    wh, ww = _pair(window, 'window')
    if weights not in WEIGHT_MODES:
        raise ValueError('window weights %r: one of %s' % (weights, list(WEIGHT_MODES)))
    if weights == 'uniform':
        return torch.ones(wh, dtype=torch.float32), torch.ones(ww, dtype=torch.float32)
    sigma_scale = float(sigma_scale)
    if not sigma_scale > 0.0:
        raise ValueError('sigma_scale %r: a positive number expected' % (sigma_scale,))

    def axis(win):
        i = torch.arange(win, dtype=torch.float64)
        return torch.exp(-0.5 * ((i - (win - 1) / 2.0) / (sigma_scale * win)) ** 2).to(torch.float32)
    gh, gw = axis(wh), axis(ww)
    # a corner of the image is covered by one window only: its weight g_h[0] * g_w[0] must not underflow, or den = 0 there
    if float(gh[0] * gw[0]) < torch.finfo(torch.float32).tiny:
        raise ValueError('sigma_scale %r: the corner weight of a %d x %d window is no normal fp32 number (%.3g); about 0.054 '
                         'is the least that works' % (sigma_scale, wh, ww, float(gh[0].double() * gw[0].double())))
    return gh, gw


@functools.lru_cache(maxsize=16)
def _device_weights(window, weights, sigma_scale, device):
    return tuple(g.to(device) for g in window_weights(window, weights, sigma_scale))


def _int_array(values):
    return (ctypes.c_int * len(values))(*values)


def window_stack(x, window, stride=None):
    """[N,C,H,W] fp32 -> [B,N,C,wh,ww]: plane b is window b of `window_grid(H, W, window, stride)` of every image, rows and
    columns beyond the image clamped to its last.  HIP tensors: one launch of `aide_window_stack`; CPU tensors: torch
    indexing, the definition."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError('window_stack: a [N,C,H,W] fp32 tensor expected')
    n, c, h, w = x.shape
    if min(n, c, h, w) < 1:
        raise ValueError('window_stack: an empty tensor %s' % (tuple(x.shape),))
    wh, ww = _pair(window, 'window')
    sy, sx = window_grid(h, w, (wh, ww), stride)
    b = len(sy) * len(sx)
    x = x.detach()
    if not x.is_cuda:
        rows, cols = torch.arange(wh), torch.arange(ww)
        return torch.stack([x[:, :, (rows + y0).clamp(max=h - 1)][:, :, :, (cols + x0).clamp(max=w - 1)] for y0 in sy for x0 in sx])
    if max(n * c * h * w, b * n * c * wh * ww) >= 2 ** 31:
        raise ValueError('window_stack: %d windows of %d x %d x %d x %d, fewer than 2^31 elements expected' % (b, n, c, wh, ww))
    if not x.is_contiguous():
        x = x.contiguous()
    y = torch.empty(b, n, c, wh, ww, device=x.device, dtype=torch.float32)
    check(lib.aide_window_stack(ptr(x), c * h * w, ptr(y), c * wh * ww, n, c, h, w, wh, ww, _int_array(sy), len(sy),
                                _int_array(sx), len(sx), stream_ptr()), 'window_stack')
    return y


def _blend_args(values, image_size, window, stride):
    """-> (values as [B,N,C,wh,ww], (h, w), (wh, ww), starts_y, starts_x), checked"""
    h, w = _pair(tuple(image_size), 'image_size')
    wh, ww = _pair(window, 'window')
    sy, sx = window_grid(h, w, (wh, ww), stride)
    b = len(sy) * len(sx)
    if values.dim() not in (4, 5) or values.dtype != torch.float32:
        raise ValueError('window_blend: [B,N,C,wh,ww] or [B*N,C,wh,ww] fp32 values expected')
    if values.dim() == 4:
        if values.shape[0] < b or values.shape[0] % b:
            raise ValueError('window_blend: %d window images, a positive multiple of the %d windows of the grid expected'
                             % (values.shape[0], b))
        values = values.reshape((b, values.shape[0] // b) + tuple(values.shape[1:]))
    if values.shape[0] != b or values.shape[1] < 1:
        raise ValueError('window_blend: values of %d windows, the grid of a %d x %d image has %d' % (values.shape[0], h, w, b))
    if tuple(values.shape[-2:]) != (wh, ww):
        raise ValueError('window_blend: values of %d x %d pixels for a %d x %d window' % (tuple(values.shape[-2:]) + (wh, ww)))
    if not 2 <= values.shape[2] <= MAX_CLASSES:
        raise ValueError('window_blend: %d classes, 2 .. %d are supported' % (values.shape[2], MAX_CLASSES))
    if max(values.numel(), values.shape[1] * values.shape[2] * h * w) >= 2 ** 31:
        raise ValueError('window_blend: %d values, fewer than 2^31 expected' % values.numel())
    return values.detach(), (h, w), (wh, ww), sy, sx


def _blend_host(values, hw, win, sy, sx, gh, gw, logits, probs):
    (h, w), (wh, ww) = hw, win
    _, n, c = values.shape[:3]
    acc = torch.zeros(n, c, h, w, dtype=torch.float32, device=values.device)
    den = torch.zeros(n, 1, h, w, dtype=torch.float32, device=values.device)
    gh, gw = gh.to(values.device), gw.to(values.device)
    for b, (y0, x0) in enumerate((y0, x0) for y0 in sy for x0 in sx):
        hh, wv = min(wh, h - y0), min(ww, w - x0)                # the part of the window inside the image
        z = values[b, :, :, :hh, :wv]
        if logits:
            e = torch.exp(z - z.max(1, keepdim=True).values)
            s = e[:, 0:1]
            for k in range(1, c):
                s = s + e[:, k:k + 1]
            p = e * (1.0 / s)
        else:
            p = z
        wgt = gh[:hh, None] * gw[None, :wv]
        acc[:, :, y0:y0 + hh, x0:x0 + wv] = acc[:, :, y0:y0 + hh, x0:x0 + wv] + wgt * p
        den[:, :, y0:y0 + hh, x0:x0 + wv] = den[:, :, y0:y0 + hh, x0:x0 + wv] + wgt
    best = acc[:, 0]
    labels = torch.zeros(best.shape, dtype=torch.int64, device=acc.device)
    for k in range(1, c):
        gt = acc[:, k] > best
        best = torch.where(gt, acc[:, k], best)
        labels[gt] = k
    return (labels, acc / den) if probs else labels


def window_blend_host(values, image_size, window, stride=None, weights='gaussian', sigma_scale=0.125, logits=True, probs=False):
    """The host statement of `aide_window_blend` in torch, operation for operation in fp32: per window b (in order), on the
    part of it inside the image, p = the soft-max as `ensemble_vote_host` takes it (m = max_c z, e_c = exp(z_c - m), s = e_0 +
    e_1 + ..., p_c = e_c * (1 / s)) or the values themselves (logits=False); w = g_h[u] * g_w[v]; acc_c = acc_c + w * p_c;
    den = den + w; label = the first class of the largest acc_c; probs = acc / den."""
    values, hw, win, sy, sx = _blend_args(values, image_size, window, stride)
    gh, gw = window_weights(win, weights, sigma_scale)
    return _blend_host(values, hw, win, sy, sx, gh, gw, logits, probs)


def window_blend(values, image_size, window, stride=None, weights='gaussian', sigma_scale=0.125, logits=True, probs=False):
    """Window maps [B,N,C,wh,ww] (or [B*N,C,wh,ww], window-major) of the grid of an image_size = (H, W) image, fp32 logits
    (logits=True) or probabilities, C = 2 .. 8 -> int64 labels [N,H,W], with probs=True also the blended probabilities fp32
    [N,C,H,W].  HIP tensors: one launch of `aide_window_blend`; CPU tensors: `window_blend_host`."""
    values, (h, w), (wh, ww), sy, sx = _blend_args(values, image_size, window, stride)
    if not values.is_cuda:
        gh, gw = window_weights((wh, ww), weights, sigma_scale)
        return _blend_host(values, (h, w), (wh, ww), sy, sx, gh, gw, logits, probs)
    gh, gw = _device_weights((wh, ww), weights, float(sigma_scale), values.device)
    if not values.is_contiguous():
        values = values.contiguous()
    _, n, c = values.shape[:3]
    labels = torch.empty(n, h, w, device=values.device, dtype=torch.int64)
    pr = torch.empty(n, c, h, w, device=values.device, dtype=torch.float32) if probs else None
    check(lib.aide_window_blend(ptr(values), int(bool(logits)), c * wh * ww, n, c, h, w, wh, ww, _int_array(sy), len(sy),
                                _int_array(sx), len(sx), ptr(gh), ptr(gw), ptr(labels), ptr(pr), c * h * w, stream_ptr()),
          'window_blend')
    return (labels, pr) if probs else labels


def predict_windows(nets, modal_inputs, window, stride=None, weights='gaussian', sigma_scale=0.125, views=None, batch_size=16,
                    probs=False):
    """`predict_labels(..., window=...)`: int64 labels [S,H,W] (and the blended probabilities [S,C,H,W]) of S slices of any size
    H x W from windows of the training size; wh and ww must be multiples of 16 (the networks halve the grid four times),
    quarter-turn views need wh == ww.  With B windows per slice and V views (1 without views), slices go in groups of g =
    max(1, batch_size // (B * V)); a group's window stack [B,g,...] is forwarded in consecutive chunks of at most max(1,
    batch_size // V) window images, in stack order, into one [B,g,C,wh,ww] buffer, and blended by one launch.  One network and
    no views: the buffer holds logits.  Views or several networks: every chunk goes through `member_logits` and
    `ensemble_vote(..., probs=True)`, the buffer holds their mean soft-max maps and the blend takes probabilities."""
    nets = _net_list(nets)
    if not modal_inputs:
        raise TypeError('predict_windows: no input')
    wh, ww = _pair(window, 'window')
    if wh % 16 or ww % 16:
        raise ValueError('predict_windows: a %d x %d window, multiples of 16 expected' % (wh, ww))
    codes = (0,) if views is None else view_codes(views, wh, ww)
    _member_count(nets, codes)
    voted = views is not None or len(nets) > 1
    for m in modal_inputs:
        if m.dim() != 4 or m.dtype != torch.float32 or m.shape[0] < 1 or (m.shape[0],) + tuple(m.shape[-2:]) != \
                (modal_inputs[0].shape[0],) + tuple(modal_inputs[0].shape[-2:]):
            raise ValueError('predict_windows: the inputs are [S,3,H,W] fp32 tensors of one slice count and size, got %s'
                             % ', '.join('%s %s' % (tuple(t.shape), t.dtype) for t in modal_inputs))
    s, _, h, w = modal_inputs[0].shape
    sy, sx = window_grid(h, w, (wh, ww), stride)
    window_weights((wh, ww), weights, sigma_scale)                # an unknown mode raises before any forward
    b, v = len(sy) * len(sx), len(codes)
    group = max(1, int(batch_size) // (b * v))
    chunk = max(1, int(batch_size) // v)
    dev = next(nets[0].parameters()).device
    labels, pr = [], []
    with torch.no_grad():
        for i in range(0, s, group):
            stacks = [window_stack(m[i:i + group].to(dev, non_blocking=True), (wh, ww), stride) for m in modal_inputs]
            g = stacks[0].shape[1]
            stacks = [t.view((b * g,) + tuple(t.shape[2:])) for t in stacks]
            buf = None
            for j in range(0, b * g, chunk):
                xs = [t[j:j + chunk] for t in stacks]
                if voted:
                    outs, member_codes = member_logits(nets, xs, codes)
                    z = ensemble_vote([o[k] for o in outs for k in range(v)], member_codes, probs=True)[1]
                else:
                    z = nets[0](*xs).detach()
                    if z.dim() != 4 or z.shape[0] != xs[0].shape[0] or tuple(z.shape[-2:]) != (wh, ww):
                        raise RuntimeError('predict_windows: the network returned %s for a batch of %s'
                                           % (tuple(z.shape), tuple(xs[0].shape)))
                if buf is None:
                    buf = torch.empty((b * g,) + tuple(z.shape[1:]), device=z.device, dtype=torch.float32)
                buf[j:j + chunk].copy_(z)
            r = window_blend(buf.view((b, g) + tuple(buf.shape[1:])), (h, w), (wh, ww), stride, weights, sigma_scale,
                             logits=not voted, probs=probs)
            labels.append(r[0] if probs else r)
            if probs:
                pr.append(r[1])
    labels = torch.cat(labels, 0) if len(labels) > 1 else labels[0]
    if not probs:
        return labels
    return labels, (torch.cat(pr, 0) if len(pr) > 1 else pr[0])
