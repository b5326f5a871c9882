"""Shared inputs and the float64 statement of the sliding-window tests (tests/test_window_host.py, tests/test_gpu_window.py),
written out here so that the tests do not lean on the code under test.

A case is (N, C, H, W, window, stride, weights): random logits `3 * randn` of shape [B,N,C,wh,ww], one map per window of the
grid of an H x W image.  The grid along an axis: [0] when size <= win, else [0, s, 2 s, ... < size - win] + [size - win]; window
b = a_y * nx + a_x.  The cases: a regular 2 x 2-fold overlap; stride = window with a clamped last window on both axes; a
single window; an image lower than the window (padding rows that are never read back); an irregular last stride; a
non-square window with a 3 x 3-fold overlap.

Bounds.  PROB_TOL = 2e-6 absolute on the blended probability against float64: the blend is a convex combination of
soft-maxes, each good to a few ulp of 1 (2^-24 = 6e-8 each for the subtraction, the exponential, the sum, the reciprocal and
the product); with at most 16 covering windows (asserted below for every case) the accumulations of acc and den add at most
16 roundings of 6e-8 relative each, the weight product and the division one more each -- the budget ensemble_cases derives
for 16 members.  Labels must be equal at every pixel: every case is asserted to have a float64 top-two gap of the blended
probability above MIN_GAP = 1e-5 everywhere, five times the bound, so no pixel is excused."""
import functools
import math

import torch

PROB_TOL = 2e-6
MIN_GAP = 1e-5
MAX_COVER = 16

# N, C, H, W, window, stride, weights, seed offset (0 unless the case's smallest gap asked for another draw)
CASES = [
    (2, 2, 40, 56, (16, 16), (8, 8), 'gaussian', 1),
    (1, 5, 37, 45, (16, 32), (16, 32), 'uniform', 0),
    (3, 8, 16, 16, (16, 16), (8, 8), 'gaussian', 0),
    (2, 3, 9, 23, (16, 16), (8, 8), 'gaussian', 0),
    (1, 2, 70, 33, (32, 32), (12, 12), 'gaussian', 0),
    (2, 4, 50, 50, (32, 16), (10, 6), 'uniform', 2),
]
IDS = ['overlap2x2-c2-40x56', 'abutting-c5-37x45', 'single-c8-16', 'padded-c3-9x23', 'irregular-c2-70x33', 'overlap3x3-c4-50']
SIGMA_SCALE = 0.125


def starts(size, win, stride):
    if size <= win:
        return [0]
    out, k = [], 0
    while k * stride < size - win:
        out.append(k * stride)
        k += 1
    return out + [size - win]


def grid(h, w, window, stride):
    """-> [(sy, sx)] of the windows in raster order"""
    return [(y0, x0) for y0 in starts(h, window[0], stride[0]) for x0 in starts(w, window[1], stride[1])]


def stack(x, window, stride):
    """the clamped window stack [B,N,C,wh,ww] of x [N,C,H,W], element by index"""
    h, w = x.shape[-2:]
    planes = []
    for y0, x0 in grid(h, w, window, stride):
        rows = torch.tensor([min(y0 + u, h - 1) for u in range(window[0])])
        cols = torch.tensor([min(x0 + v, w - 1) for v in range(window[1])])
        planes.append(x.index_select(-2, rows).index_select(-1, cols))
    return torch.stack(planes)


def axis_weights(win, weights):
    """the fp32 axis weights: float64 values rounded once"""
    if weights == 'uniform':
        return torch.ones(win, dtype=torch.float32)
    return torch.tensor([math.exp(-0.5 * ((i - (win - 1) / 2.0) / (SIGMA_SCALE * win)) ** 2) for i in range(win)],
                        dtype=torch.float64).float()


def coverage(h, w, window, stride):
    """how many windows contain each pixel, int64 [H,W]"""
    cnt = torch.zeros(h, w, dtype=torch.int64)
    for y0, x0 in grid(h, w, window, stride):
        cnt[y0:y0 + window[0], x0:x0 + window[1]] += 1
    return cnt


def blend_f64(values, h, w, window, stride, weights, logits=True):
    """float64 statement: per window torch.softmax in float64 (or the values themselves), float64 products of the fp32 axis
    weights, weighted mean over the covering windows, arg-max -> (labels int64 [N,H,W], probs float64 [N,C,H,W], the smallest
    top-two gap of the blended probability)"""
    _, n, c = values.shape[:3]
    gh, gw = axis_weights(window[0], weights).double(), axis_weights(window[1], weights).double()
    acc = torch.zeros(n, c, h, w, dtype=torch.float64)
    den = torch.zeros(h, w, dtype=torch.float64)
    for b, (y0, x0) in enumerate(grid(h, w, window, stride)):
        hh, wv = min(window[0], h - y0), min(window[1], w - x0)
        p = values[b].double()
        p = (torch.softmax(p, 1) if logits else p)[:, :, :hh, :wv]
        wgt = gh[:hh, None] * gw[None, :wv]
        acc[:, :, y0:y0 + hh, x0:x0 + wv] += wgt * p
        den[y0:y0 + hh, x0:x0 + wv] += wgt
    p = acc / den
    top = p.topk(2, dim=1).values
    return p.argmax(1), p, float((top[:, 0] - top[:, 1]).min())


@functools.lru_cache(maxsize=None)
def case_logits(idx):
    """z [B,N,C,wh,ww] fp32 on the CPU (shared, never modified)"""
    N, C, H, W, window, stride, weights, off = CASES[idx]
    cover = coverage(H, W, window, stride)
    assert 1 <= int(cover.min()) and int(cover.max()) <= MAX_COVER, (idx, int(cover.min()), int(cover.max()))
    B = len(grid(H, W, window, stride))
    g = torch.Generator().manual_seed(4321 + 100 * idx + C + off)
    return (3 * torch.randn(B, N, C, window[0], window[1], generator=g)).float()


@functools.lru_cache(maxsize=None)
def case_reference(idx):
    N, C, H, W, window, stride, weights, off = CASES[idx]
    return blend_f64(case_logits(idx), H, W, window, stride, weights)


# (H, W, window, stride): 'uniform' weights and overlap along one axis only, so coverage is 1 or 2 and p + p and the division by
# 2 are exact: stacking a map and blending it gives the bits of the map's own soft-max.  The third has padded rows.
EXACT = [(40, 32, (16, 16), (8, 16)), (32, 48, (16, 16), (16, 8)), (9, 40, (16, 16), (8, 16)), (48, 48, (32, 16), (16, 16))]


@functools.lru_cache(maxsize=None)
def exact_logits(idx):
    """L [2,5,H,W] fp32 on the CPU for EXACT[idx] (shared, never modified)"""
    H, W, window, stride = EXACT[idx]
    cover = coverage(H, W, window, stride)
    assert int(cover.min()) >= 1 and int(cover.max()) <= 2
    g = torch.Generator().manual_seed(977 + idx)
    return (3 * torch.randn(2, 5, H, W, generator=g)).float()
