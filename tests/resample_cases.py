"""Inputs of the resampling tests (test_resample_host.py, test_gpu_resample.py): the geometries, each chosen because it can go
wrong in its own way, seeded label volumes and images, and the two references that do not come from aide_amd: scipy's zoom of
the one-hot planes and the block-majority rule of the halving geometry."""
import numpy as np

GEOMETRIES = (
    ((5, 7, 6), (9, 11, 13)),          # generic up-sampling
    ((7, 9, 11), (3, 5, 4)),           # generic down-sampling
    ((12, 10, 33), (17, 14, 33)),      # the slice axis is an identity, in-plane generic
    ((1, 9, 7), (1, 13, 4)),           # a single slice
    ((4, 5, 3), (8, 10, 6)),           # x 2: weights 1/4 and 3/4, exact
    ((8, 6, 10), (4, 3, 5)),           # / 2: every corner weighs exactly 1/8, ties everywhere
    ((3, 4, 5), (3, 4, 5)),            # identity
    ((1, 1, 1), (4, 3, 2)),            # everything clamped
    ((6, 40, 70), (9, 61, 131)),       # crosses workgroup and row boundaries; 131 is no multiple of the per-thread vector
)
IDS = ['%dx%dx%d-%dx%dx%d' % (d + e) for d, e in GEOMETRIES]
HALVING = 5                            # its index
CAPPED = (0, 2, 3, 4, 8)               # the generic and x 2 geometries: scipy's margin may exclude at most 2 % of their voxels
CLASSES = (2, 3, 5, 8)
MARGIN = 1e-9


def label_volume(shape, c, dtype=np.int64, seed=0):
    """a smoothed-noise arg-max map with c classes; about 0.5 % of the voxels hold a value >= c, and an int64 volume one negative"""
    from scipy import ndimage
    rng = np.random.default_rng(1000 * seed + 10 * c + sum(shape))
    planes = np.stack([ndimage.uniform_filter(rng.normal(size=shape), size=5, mode='nearest') for _ in range(c)])
    vol = planes.argmax(0).astype(dtype)
    stray = rng.random(shape) < 0.005
    vol[stray] = c + rng.integers(0, 3, size=shape)[stray]
    if dtype == np.int64:
        vol.reshape(-1)[vol.size // 2] = -3
    if vol.size > 4:
        vol.reshape(-1)[1] = c                      # at least one stray value whatever the seed
    return vol


def image(shape, seed=0):
    rng = np.random.default_rng(77 + seed + sum(shape))
    return (rng.normal(size=shape) * 1000.0).astype(np.float32)


def probabilities(shape, c, seed=0):
    """[S,C,H,W] float32: a soft-max of smoothed noise"""
    s, h, w = shape
    rng = np.random.default_rng(5 + seed + 10 * c + sum(shape))
    z = rng.normal(size=(s, c, h, w)) * 2.0
    p = np.exp(z - z.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def zoom(x, e, order=1):
    """scipy's resampling of one float64 volume onto the shape e"""
    from scipy import ndimage
    return ndimage.zoom(x, [m / n for n, m in zip(x.shape, e)], order=order, mode='nearest', grid_mode=True)


def scipy_labels(vol, e, c):
    """-> (labels, decided): the arg-max of the c zoomed one-hot planes and where the best class sum beats the second by MARGIN"""
    planes = np.stack([zoom((vol == k).astype(np.float64), e) for k in range(c)])
    assert planes.shape[1:] == tuple(e)
    ranked = np.sort(planes, axis=0)
    return planes.argmax(0), ranked[-1] - ranked[-2] > MARGIN


def block_majority(vol, c):
    """the exact rule of the halving geometry: the most frequent in-range value of every 2 x 2 x 2 block, the lowest class on a
    tie, 0 when no value is in range"""
    d0, d1, d2 = vol.shape
    blocks = vol.reshape(d0 // 2, 2, d1 // 2, 2, d2 // 2, 2).transpose(0, 2, 4, 1, 3, 5).reshape(d0 // 2, d1 // 2, d2 // 2, 8)
    counts = np.stack([(blocks == k).sum(-1) for k in range(c)])
    return counts.argmax(0).astype(np.uint8)          # numpy's argmax returns the first of equal integer counts
