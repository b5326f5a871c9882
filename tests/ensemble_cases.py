"""Shared inputs and the float64 statement of the ensemble tests (tests/test_ensemble_host.py, tests/test_gpu_ensemble.py).

A case is (K, N, C, H, W, views): K members' random logits `z[k]`, member k in the frame of view `codes[k]`.  36, 20 x 52, 17
and 9 x 23 are no multiples of the kernels' 32-pixel tile, and two of them are odd.

Bounds.  PROB_TOL = 2e-6 absolute on the mean probability against float64: one fp32 soft-max is good to a few ulp of 1
(2^-24 = 6e-8 each for the subtraction, the exponential, the sum, the reciprocal and the product), and adding at most 16 of
them costs at most 15 roundings at a magnitude of at most 16 (16 * 6e-8 = 1e-6 each before the division by K, i.e. at
most 15 * 1e-6 / 16 after it), so 2e-6 covers both.  Labels must be equal at every pixel: every case is asserted to have a
float64 top-two gap of the mean probability above MIN_GAP = 1e-5 everywhere, five times the bound, so no pixel is excused."""
import functools

import torch

PROB_TOL = 2e-6
MIN_GAP = 1e-5

D4 = (0, 1, 2, 3, 4, 5, 6, 7)
# K, N, C, H, W, member codes, seed offset (0 unless the case's smallest gap asked for another draw)
CASES = [
    (8, 3, 2, 36, 36, D4, 0),
    (8, 3, 5, 36, 36, D4, 0),
    (4, 2, 3, 20, 52, (0, 4, 2, 6), 0),
    (16, 2, 8, 17, 17, D4 + D4, 0),
    (2, 2, 2, 9, 23, (0, 4), 0),
]
IDS = ['d4-c2-36', 'd4-c5-36', 'flip4-c3-20x52', 'd4x2-c8-17', 'flip2-c2-9x23']
SHAPES = [(3, 36, 36), (3, 36, 36), (2, 20, 52), (2, 17, 17), (2, 9, 23)]       # (N, H, W) of the five cases


def view_apply(x, code):
    """the definition, written out here so that the tests do not lean on the code under test"""
    return torch.rot90(torch.flip(x, [-1]) if code & 4 else x, code & 3, (-2, -1))


def view_invert(y, code):
    x = torch.rot90(y, -(code & 3), (-2, -1))
    return torch.flip(x, [-1]) if code & 4 else x


def valid_codes(h, w):
    return D4 if h == w else (0, 2, 4, 6)


@functools.lru_cache(maxsize=None)
def case_logits(idx):
    """z [K,N,C,H,W] fp32 on the CPU (member k in the frame of codes[k]; shared, never modified) and the codes"""
    K, N, C, H, W, codes, off = CASES[idx]
    g = torch.Generator().manual_seed(1234 + 100 * K + C + off)
    z = (3 * torch.randn(K, N, C, H, W, generator=g)).float()
    return z, codes


def vote_f64(z, codes):
    """float64 statement: inverse views, soft-max, mean, arg-max -> (labels int64 [N,H,W], probs float64 [N,C,H,W],
    the smallest top-two gap of the mean probability)"""
    p = torch.stack([torch.softmax(view_invert(z[k].double(), codes[k]), 1) for k in range(len(codes))]).mean(0)
    top = p.topk(2, dim=1).values
    return p.argmax(1), p, float((top[:, 0] - top[:, 1]).min())


@functools.lru_cache(maxsize=None)
def case_reference(idx):
    z, codes = case_logits(idx)
    return vote_f64(z, codes)
