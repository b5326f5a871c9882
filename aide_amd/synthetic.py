"""Synthetic CHAOS-shaped batches (no dataset I/O on the hot path).

Reproduces the *tensor contract* of the reference loader, not its file I/O:
  datasetchaos_comparison/dataset.py:24-25   grayscale slice replicated to 3 channels
  datasetchaos_comparison/transform.py:128   /255
  datasetchaos_comparison/transform.py:160-163  per-image per-channel standardise, unbiased std
  datasetchaos_comparison/dataset.py:63-67 + trainchaos_comparison_1case.py:194
      targets = one-hot mask channel 1 -> int64 {0,1} [N,H,W]
Statistics follow SURVEY.md §8(d): ~28 % exact-zero background, ~12 % saturated pixels,
one smooth foreground blob (0-14 % of the slice), ~40 % of slices empty.
"""
import numpy as np
import torch


def _smooth_field(rng, size, coarse=8):
    """Bilinear-upsampled coarse noise in [0,1] (numpy only)."""
    g = rng.rand(coarse + 1, coarse + 1)
    xs = np.linspace(0, coarse, size, endpoint=False)
    i0 = np.floor(xs).astype(np.int64)
    f = (xs - i0)[None, :]
    rows = g[:, i0] * (1 - f) + g[:, i0 + 1] * f            # [coarse+1, size]
    fy = (xs - i0)[:, None]
    return rows[i0, :] * (1 - fy) + rows[i0 + 1, :] * fy     # [size, size]


def chaos_slice(rng, size):
    """One (in-phase u8, out-phase u8, liver mask {0,1}) triple, HxW."""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    cy, cx = size * (0.5 + 0.04 * rng.randn()), size * (0.5 + 0.04 * rng.randn())
    ry, rx = size * 0.46, size * 0.50
    body = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0      # ~72 % of the slice
    f = _smooth_field(rng, size)
    tex = 0.06 * rng.randn(size, size)
    g1 = np.clip(255.0 * (0.10 + 1.33 * f + tex), 0, 255)            # ~12 % saturate
    g2 = np.clip(255.0 * (0.05 + 1.10 * f + 0.08 * rng.randn(size, size)), 0, 255)
    g1 = np.where(body, g1, 0.0).round().astype(np.uint8)
    g2 = np.where(body, g2, 0.0).round().astype(np.uint8)
    mask = np.zeros((size, size), np.int64)
    if rng.rand() >= 0.4:                                            # ~40 % empty slices
        frac = rng.uniform(0.005, 0.14)
        r = np.sqrt(frac / np.pi) * size
        by = cy + rng.uniform(-0.15, 0.15) * size
        bx = cx - rng.uniform(0.05, 0.25) * size
        ang = rng.uniform(0, np.pi)
        dy, dx = yy - by, xx - bx
        u = dy * np.cos(ang) + dx * np.sin(ang)
        v = -dy * np.sin(ang) + dx * np.cos(ang)
        mask = ((u / (1.3 * r)) ** 2 + (v / (0.77 * r)) ** 2 <= 1.0) & body
        mask = mask.astype(np.int64)
    return g1, g2, mask


def _to_tensor_norm(g):
    """u8 HxW -> float32 [3,H,W]: replicate, /255, standardise with unbiased std."""
    x = torch.from_numpy(g.astype(np.float32) / 255.0)
    x = x.unsqueeze(0).expand(3, -1, -1).contiguous()
    mean = x.mean(dim=(1, 2), keepdim=True)
    std = x.std(dim=(1, 2), keepdim=True)           # unbiased (transform.py:160-163)
    return (x - mean) / std


def chaos_batch(n, size=256, seed=1234, single_modal=False):
    """Returns (inphase[N,3,H,W] f32, outphase[N,3,H,W] f32, targets[N,H,W] i64) on CPU."""
    rng = np.random.RandomState(seed)
    a, b, t = [], [], []
    for _ in range(n):
        g1, g2, m = chaos_slice(rng, size)
        a.append(_to_tensor_norm(g1))
        b.append(_to_tensor_norm(g2))
        t.append(torch.from_numpy(m))
    inphase, outphase, targets = torch.stack(a), torch.stack(b), torch.stack(t)
    if single_modal:
        return inphase, None, targets
    return inphase, outphase, targets


CHAOS_LIVER = 63      # the liver's byte in the CHAOS mask PNGs (datasetchaos_proposed/dataset.py:9, palette[1])


def chaos_cases(n_cases, size=256, seed=1234, slices=(3, 7), labelled=(0,), single_modal=False):
    """A fixed synthetic case set for the label-refresh loop: K cases of ragged slice counts (uniform in `slices`, inclusive),
    their slices concatenated.  -> dict(inphase / outphase f32 [S,3,H,W] (outphase None when single_modal), truth u8 [S,H,W]
    (the mask PNG bytes: CHAOS_LIVER on the liver), initial u8 [S,H,W] (the truth for the labelled cases; for the others a
    noisy pseudo-label: the truth shifted by a few pixels, with some slices emptied), slice_start [K + 1], labelled)."""
    rng = np.random.RandomState(seed)
    a, b, truth, initial, start = [], [], [], [], [0]
    for k in range(n_cases):
        ns = int(rng.randint(slices[0], slices[1] + 1))
        dy, dx = (int(v) for v in rng.randint(-max(1, size // 16), max(1, size // 16) + 1, 2))
        for _ in range(ns):
            g1, g2, m = chaos_slice(rng, size)
            a.append(_to_tensor_norm(g1))
            if not single_modal:
                b.append(_to_tensor_norm(g2))
            m = (m * CHAOS_LIVER).astype(np.uint8)
            truth.append(m)
            noisy = np.roll(m, (dy, dx), (0, 1)) if rng.rand() >= 0.2 else np.zeros_like(m)
            initial.append(m if k in labelled else noisy)
        start.append(start[-1] + ns)
    return dict(inphase=torch.stack(a), outphase=None if single_modal else torch.stack(b),
                truth=torch.from_numpy(np.stack(truth)), initial=torch.from_numpy(np.stack(initial)),
                slice_start=start, labelled=[k for k in labelled if k < n_cases])


def chaos_cases_multiorgan(n_cases, num_classes=5, size=256, seed=1234, slices=(3, 7), labelled=(0,)):
    """`chaos_cases` for multi-organ masks: the same dict, with truth / initial carrying the bytes CHAOS_PALETTE[:num_classes]
    (num_classes = 2 .. 5).  Organ c = 1 .. num_classes - 1 is an ellipsoid around its own point of a ring about the body
    centre, so the organs of a case are disjoint blobs through its slices (a pixel takes the first organ that covers it);
    every case but the first lacks each organ with probability 0.25 (some cases lack an organ altogether, and the first case
    has them all).  initial: the truth for the labelled cases; for the others the truth shifted by a few pixels with some
    slices emptied, and sometimes one organ missing from the pseudo-label."""
    from .labelbank import CHAOS_PALETTE      # background, liver, right / left kidney, spleen
    if not 2 <= num_classes <= len(CHAOS_PALETTE):
        raise ValueError('chaos_cases_multiorgan: num_classes 2 .. %d, got %r' % (len(CHAOS_PALETTE), num_classes))
    rng = np.random.RandomState(seed)
    organs = num_classes - 1
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    ring = 0.22 * size
    # neighbours on the ring are 2 * ring * sin(pi / organs) apart and the blobs are 1.2 times as wide as high: a longer
    # half-axis below half of that distance cannot meet its neighbour's
    rmax = min(0.16 * size, 0.45 / 1.2 * 2 * ring * np.sin(np.pi / organs) if organs > 1 else 0.16 * size)
    a, b, truth, initial, start = [], [], [], [], [0]
    for k in range(n_cases):
        ns = int(rng.randint(slices[0], slices[1] + 1))
        dy, dx = (int(v) for v in rng.randint(-max(1, size // 16), max(1, size // 16) + 1, 2))
        present = (rng.rand(organs) >= 0.25) | (k == 0)
        forgotten = int(rng.randint(0, organs)) if rng.rand() < 0.3 else -1        # an organ the pseudo-label misses
        radius = rmax * rng.uniform(0.6, 1.0, organs)
        phase = rng.uniform(0, 2 * np.pi)
        for s in range(ns):
            g1, g2, _ = chaos_slice(rng, size)
            a.append(_to_tensor_norm(g1))
            b.append(_to_tensor_norm(g2))
            m = np.zeros((size, size), np.uint8)
            z = (s + 0.5) / ns * 2 - 1                                               # -1 .. 1 through the case
            for c in range(organs):
                r2 = radius[c] ** 2 * (1 - 0.8 * z * z)                             # the ellipsoid's section in this slice
                ang = phase + 2 * np.pi * c / organs
                cy, cx = size * 0.5 + ring * np.sin(ang), size * 0.5 + ring * np.cos(ang)
                if present[c]:
                    m[(m == 0) & ((yy - cy) ** 2 + ((xx - cx) / 1.2) ** 2 <= r2)] = CHAOS_PALETTE[c + 1]
            truth.append(m)
            noisy = np.roll(m, (dy, dx), (0, 1)) if rng.rand() >= 0.2 else np.zeros_like(m)
            if forgotten >= 0:
                noisy = np.where(noisy == CHAOS_PALETTE[forgotten + 1], 0, noisy).astype(np.uint8)
            initial.append(m if k in labelled else noisy)
        start.append(start[-1] + ns)
    return dict(inphase=torch.stack(a), outphase=torch.stack(b),
                truth=torch.from_numpy(np.stack(truth)), initial=torch.from_numpy(np.stack(initial)),
                slice_start=start, labelled=[k for k in labelled if k < n_cases])
