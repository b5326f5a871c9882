"""Shared by test_surface_host.py and test_gpu_surface.py: two independent float64 statements of the surface-distance
definitions (aide_amd/utils/metrics3d.py), seeded case generators, and the derived tolerances.

reference()  scipy: binary_erosion for the border, distance_transform_edt for the distances
brute()      numpy only, O(n_P * n_T): the border from shifted comparisons, every pair of border voxels evaluated
Both form, per distance, three rounded products sp_k * delta_k, three rounded squares, two rounded adds and one correctly
rounded sqrt of non-negative terms: at most 4 ulp each from the true value, so two implementations of that recipe (the device
is a third) are at most 8 ulp = 2^-50 apart; REL = 2^-49 leaves a factor 2.  This covers a near-tie between two candidates
that is decided on rounded values.  With spacing (1, 1, 1) every squared distance is an integer below 2^53: results are
bit-equal."""
import math

import numpy as np

REL = 2.0 ** -49
SPACINGS = ((1.0, 1.0, 1.0), (0.7, 0.7, 5.5), (1.37, 1.37, 7.7))
SMALL_SHAPES = ((5, 37, 19), (1, 7, 1), (33, 1, 40), (17, 31, 16))
# The edges of the min-plus walk (csrc/surface3d.hip), which the surface scores and the distance transform share: it takes the
# lines along d1 and then along d0 in chunks of 32 candidates and 32 results, 64 neighbouring lines (columns) per workgroup.
# Line lengths 1, 31, 32, 33, 65 on both axes: below, at and past a chunk, and a second chunk; column counts 1, 63, 64, 65 in
# both passes (d0 * d2 along d1, d1 * d2 along d0): a partial workgroup, a full one, and a second one.
EDGE_SHAPES = ((33, 1, 1), (65, 1, 2), (1, 33, 1), (2, 65, 1), (31, 9, 7), (32, 1, 64), (1, 1, 65), (9, 31, 7), (64, 32, 1))
for _axis in (0, 1):                              # a condition on the chosen inputs
    assert {1, 31, 32, 33, 65} <= {s[_axis] for s in EDGE_SHAPES}
    assert {1, 63, 64, 65} <= {s[1 - _axis] * s[2] for s in EDGE_SHAPES}


def _fg(x, cls):
    x = np.asarray(x)
    return (x != 0) if cls is None or cls < 0 else (x == cls)


def _pack(bp, bt, fp, ft, dist):
    """the eight raw values + the two maps from the borders, the foregrounds and dist = (D_T on bp, D_P on bt) or None"""
    maps = [np.full(bp.shape, -1.0, np.float64) for _ in range(2)]
    s, m = [0.0, 0.0], [0.0, 0.0]
    if dist is not None:
        for k, b in enumerate((bp, bt)):
            maps[k][b] = dist[k]
            s[k], m[k] = math.fsum(dist[k].tolist()), float(dist[k].max())
    return dict(n_P=int(bp.sum()), n_T=int(bt.sum()), V_P=int(fp.sum()), V_T=int(ft.sum()), S_PT=s[0], S_TP=s[1], M_PT=m[0],
                M_TP=m[1], dist_P=maps[0], dist_T=maps[1])


def reference(pred, target, spacing, cls=None):
    from scipy import ndimage
    fp, ft = _fg(pred, cls), _fg(target, cls)
    st = ndimage.generate_binary_structure(3, 1)
    bp, bt = (f & ~ndimage.binary_erosion(f, st, border_value=0) for f in (fp, ft))
    dist = None
    if bp.any() and bt.any():
        dist = (ndimage.distance_transform_edt(~bt, sampling=spacing)[bp],
                ndimage.distance_transform_edt(~bp, sampling=spacing)[bt])
    return _pack(bp, bt, fp, ft, dist)


def _border_np(f):
    q = np.pad(f, 1, constant_values=False)
    inner = (q[:-2, 1:-1, 1:-1] & q[2:, 1:-1, 1:-1] & q[1:-1, :-2, 1:-1] & q[1:-1, 2:, 1:-1] & q[1:-1, 1:-1, :-2]
             & q[1:-1, 1:-1, 2:])
    return f & ~inner


def _nearest(a, b, sp):
    """a [na,3], b [nb,3] integer coordinates -> float64 [na]: distance of every a to its nearest b"""
    out = np.empty(len(a), np.float64)
    step = max(1, (1 << 22) // max(1, len(b)))
    for i in range(0, len(a), step):
        d = (a[i:i + step, None, :] - b[None, :, :]).astype(np.float64) * sp
        d = d * d
        out[i:i + step] = np.sqrt(((d[..., 0] + d[..., 1]) + d[..., 2]).min(axis=1))
    return out


def brute(pred, target, spacing, cls=None):
    fp, ft = _fg(pred, cls), _fg(target, cls)
    bp, bt = _border_np(fp), _border_np(ft)
    dist = None
    if bp.any() and bt.any():
        a, b, sp = np.argwhere(bp), np.argwhere(bt), np.asarray(spacing, np.float64)   # argwhere: raster order, as bp[...]
        dist = (_nearest(a, b, sp), _nearest(b, a, sp))
    return _pack(bp, bt, fp, ft, dist)


def scores_of(raw):
    """RAVD, ASSD, MSSD from the raw values (the definitions; ASSD from the fsum values)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        ravd = np.float64(abs(raw['V_P'] - raw['V_T'])) / np.float64(raw['V_T']) * 100.0
    if raw['n_P'] == 0 or raw['n_T'] == 0:
        return ravd, np.float64('nan'), np.float64('nan')
    return ravd, np.float64(raw['S_PT'] + raw['S_TP']) / np.float64(raw['n_P'] + raw['n_T']), np.float64(max(raw['M_PT'], raw['M_TP']))


def same_float(a, b):
    a, b = np.float64(a), np.float64(b)
    return a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b))


def close(a, b, rel):
    return same_float(a, b) or abs(float(a) - float(b)) <= rel * abs(float(b))


def check_raw(got, ref, spacing, what=''):
    """`got` (any implementation: the same keys) against `ref` within the derived bounds; dist maps optional in `got`."""
    unit = tuple(spacing) == (1.0, 1.0, 1.0)
    for k in ('n_P', 'n_T', 'V_P', 'V_T'):
        assert int(got[k]) == ref[k], (what, k, got[k], ref[k])
    rel_sum = REL + (ref['n_P'] + ref['n_T']) * 2.0 ** -53
    for k in ('S_PT', 'S_TP'):
        assert close(got[k], ref[k], rel_sum), (what, k, got[k], ref[k])
    for k in ('M_PT', 'M_TP'):
        assert same_float(got[k], ref[k]) if unit else close(got[k], ref[k], REL), (what, k, got[k], ref[k])
    for k in ('dist_P', 'dist_T'):
        if got.get(k) is None:
            continue
        g, r = np.asarray(got[k], np.float64), ref[k]
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        assert np.array_equal(g >= 0, r >= 0) and np.all(g[r < 0] == -1.0), (what, k, 'set of distance entries')
        if unit:
            assert np.array_equal(g, r), (what, k, float(np.abs(g - r).max()))
        else:
            assert np.all(np.abs(g - r) <= REL * np.abs(r)), (what, k, float((np.abs(g - r) / np.maximum(np.abs(r), 1e-300)).max()))


def check_scores(got, ref, spacing, what=''):
    """a surface_scores dict (binary mode) against the raw reference values"""
    ravd, assd, mssd = scores_of(ref)
    unit = tuple(spacing) == (1.0, 1.0, 1.0)
    assert same_float(got['RAVD'], ravd), (what, got['RAVD'], ravd)
    assert close(got['ASSD'], assd, REL + (ref['n_P'] + ref['n_T']) * 2.0 ** -53), (what, got['ASSD'], assd)
    assert same_float(got['MSSD'], mssd) if unit else close(got['MSSD'], mssd, REL), (what, got['MSSD'], mssd)
    for k, r in (('n_pred', 'n_P'), ('n_target', 'n_T'), ('V_pred', 'V_P'), ('V_target', 'V_T')):
        assert int(got[k]) == ref[r], (what, k, got[k], ref[r])


# ---- cases -------------------------------------------------------------------------------------------------------------------
def random_pair(shape, density, seed, dtype=np.int64):
    rng = np.random.RandomState(seed)
    return (rng.rand(*shape) < density).astype(dtype), (rng.rand(*shape) < density).astype(dtype)


def ellipsoid_pair(shape, dtype=np.uint8):
    """a filled ellipsoid against a shifted copy with a dent"""
    z, y, x = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing='ij')
    c, r = [(s - 1) / 2.0 for s in shape], [max(1.0, 0.36 * s) for s in shape]

    def ball(cz, cy, cx, k=1.0):
        return ((z - cz) / (k * r[0])) ** 2 + ((y - cy) / (k * r[1])) ** 2 + ((x - cx) / (k * r[2])) ** 2 <= 1.0
    t = ball(*c)
    p = ball(c[0] + 0.06 * shape[0], c[1] - 0.04 * shape[1], c[2] + 0.05 * shape[2])
    p &= ~ball(c[0] + r[0], c[1], c[2], 0.4)
    return p.astype(dtype), t.astype(dtype)


def corner_blobs(n=40, dtype=np.int64):
    """a blob in one corner against a blob in the opposite one: most lines hold no border voxel"""
    p, t = np.zeros((n, n, n), dtype), np.zeros((n, n, n), dtype)
    p[:4, :3, :5] = 1
    t[-3:, -5:, -4:] = 1
    t[-1, -1, -1] = 0
    return p, t


def class_pair(shape, seed, dtype=np.int64):
    """labels for num_classes=5: class 3 is absent from both, 5 .. 7 (and for int64 also negative ones) are out of range"""
    rng = np.random.RandomState(seed)
    lut = np.array([0, 0, 0, 1, 1, 2, 2, 4, 4, 5, 6, 7, -1 if dtype == np.int64 else 200], dtype)
    p = lut[rng.randint(0, len(lut), shape)]
    t = lut[rng.randint(0, len(lut), shape)]
    # make the classes blobby, so that they have inner voxels too
    p[: shape[0] // 2, : shape[1] // 2] = 1
    t[: shape[0] // 2 + 1, 1: shape[1] // 2 + 2] = 1
    return p, t
