"""Shared by test_morphology_host.py and test_gpu_morphology.py: an independent brute-force statement of the definitions of
aide_amd/morphology.py (numpy only, no scipy call), seeded and structured cases, and the conditions on the chosen inputs.

Squared length of an integer offset o, float64, exactly this association:
    q(o) = (sp0 * o0)^2 + ((sp1 * o1)^2 + (sp2 * o2)^2)
Ball B(r) = {o : q(o) <= r * r}.  dilate(X)(v) = some o in B(r) has X(v - o) inside the volume; erode(X, outside)(v) = every o
in B(r) has X~(v + o), X~ = X inside the volume and `outside` beyond it.  The brute force loops over the offsets of the ball (in
Python, q evaluated per offset with Python floats) and, per offset, over all voxels at once by a shifted slice of the padded
volume.  Offsets with |o_k| > d_k are left out: from no voxel do they reach a voxel of the volume, and where they reach its
outside, so does the offset with every other component 0 and that one cut to +-d_k, whose q is not larger.

Exactness.  At spacing (1, 1, 1) every q and every r * r used here (r in 0, 1, 1.5, 2, 3) is a small multiple of 1/4: exact
whether or not a compiler contracts t * t + h into an fma, so the ties q == r * r (6, 6 and 30 offsets for r = 1, 2, 3) must
fall the same way everywhere.  At SPACING the device may fuse a product that the host rounds, a relative difference of at most
a few 2^-53; RADII_MM are chosen so that no offset has |q - r * r| <= 2^-40 * r * r (`gap()` asserts it at import), far outside
what either rounding can move.

Distance transform.  dist = sqrt(q) of the nearest background voxel: three rounded products, three rounded squares, two
rounded adds and one correctly rounded sqrt -- the recipe whose bound tests/surface_cases.py derives (REL = 2^-49, bit-equal
at unit spacing); it is imported from there, not restated."""
import functools
import math

import numpy as np

from surface_cases import REL, EDGE_SHAPES  # noqa: F401  (the ulp bound of the distance arithmetic; the edges of its walk)

UNIT = (1.0, 1.0, 1.0)
SPACING = (0.9, 1.3, 2.5)
RADII_UNIT = (0.0, 1.0, 1.5, 2.0, 3.0)
RADII_MM = (1.0, 2.0, 3.3, 5.5)
SETTINGS = tuple((UNIT, r) for r in RADII_UNIT) + tuple((SPACING, r) for r in RADII_MM)
OPS = ('erode0', 'erode1', 'dilate', 'open', 'close')
SHAPES = ((1, 1, 1), (3, 3, 3), (4, 16, 16), (5, 17, 33), (3, 1, 50), (67, 3, 5), (2, 67, 3), (6, 33, 18))


def q_of(o, sp):
    t0, t1, t2 = sp[0] * float(o[0]), sp[1] * float(o[1]), sp[2] * float(o[2])
    return t0 * t0 + (t1 * t1 + t2 * t2)


def reach(r, sp):
    """per axis a bound that no offset of the ball exceeds: floor(r / sp_k) + 1"""
    return tuple(int(math.floor(r / s)) + 1 for s in sp)


def offsets(r, sp, limits=None):
    """the offsets of B(r), each tested on its own; limits: |o_k| <= limits[k]"""
    w = reach(r, sp)
    if limits is not None:
        w = tuple(min(a, b) for a, b in zip(w, limits))
    found = []
    for o0 in range(-w[0], w[0] + 1):
        for o1 in range(-w[1], w[1] + 1):
            for o2 in range(-w[2], w[2] + 1):
                if q_of((o0, o1, o2), sp) <= r * r:
                    found.append((o0, o1, o2))
    return found


def gap(r, sp):
    """the smallest |q - r * r| / (r * r) over the offsets around the ball's rim"""
    w = reach(r, sp)
    best = math.inf
    for o0 in range(0, w[0] + 1):
        for o1 in range(0, w[1] + 1):
            for o2 in range(0, w[2] + 1):
                best = min(best, abs(q_of((o0, o1, o2), sp) - r * r) / (r * r))
    return best


for _r in RADII_MM:                               # a condition on the chosen inputs, from the reference alone
    assert gap(_r, SPACING) > 2.0 ** -40, (_r, gap(_r, SPACING))
TIES = {r: sum(1 for o in offsets(r, UNIT) if q_of(o, UNIT) == r * r) for r in (1.0, 2.0, 3.0)}
assert TIES == {1.0: 6, 2.0: 6, 3.0: 30}, TIES


def _shifted(xp, pad, shape, o):
    return xp[pad[0] + o[0]:pad[0] + o[0] + shape[0], pad[1] + o[1]:pad[1] + o[1] + shape[1],
              pad[2] + o[2]:pad[2] + o[2] + shape[2]]


def brute_dilate(x, r, sp):
    offs = offsets(r, sp, x.shape)
    pad = tuple(max(abs(o[k]) for o in offs) for k in range(3))
    xp = np.pad(x, [(p, p) for p in pad], constant_values=False)
    out = np.zeros(x.shape, bool)
    for o in offs:
        out |= _shifted(xp, pad, x.shape, (-o[0], -o[1], -o[2]))      # X(v - o)
    return out


def brute_erode(x, r, sp, outside):
    offs = offsets(r, sp, x.shape)
    pad = tuple(max(abs(o[k]) for o in offs) for k in range(3))
    xp = np.pad(x, [(p, p) for p in pad], constant_values=bool(outside))
    out = np.ones(x.shape, bool)
    for o in offs:
        out &= _shifted(xp, pad, x.shape, o)                          # X~(v + o)
    return out


def brute_plane(x, op, r, sp):
    if op == 'erode0':
        return brute_erode(x, r, sp, 0)
    if op == 'erode1':
        return brute_erode(x, r, sp, 1)
    if op == 'dilate':
        return brute_dilate(x, r, sp)
    if op == 'open':
        return brute_dilate(brute_erode(x, r, sp, 0), r, sp)
    assert op == 'close'
    return brute_erode(brute_dilate(x, r, sp), r, sp, 1)


def brute(vol, op, r, sp, classes=None):
    """uint8: the binary rule (classes=None) or the multi-class rule, plane by plane"""
    vol = np.asarray(vol)
    if classes is None:
        return brute_plane(vol != 0, op, r, sp).astype(np.uint8)
    out = np.zeros(vol.shape, np.uint8)
    planes = {c: brute_plane(vol == c, op, r, sp) for c in range(1, classes)}
    if op in ('erode0', 'erode1', 'open'):
        for c, p in planes.items():
            assert not (out[p] != 0).any()        # no conflict can arise
            out[p] = c
        return out
    for idx in np.ndindex(vol.shape):
        v = int(vol[idx])
        if 1 <= v < classes:
            out[idx] = v
        else:
            claim = [c for c, p in planes.items() if p[idx]]
            out[idx] = claim[0] if len(claim) == 1 else 0
    return out


def brute_distance(fg, sp):
    """float64: 0 on the background, the distance to the nearest background voxel on the foreground, +inf without any"""
    fg = np.asarray(fg, bool)
    out = np.zeros(fg.shape, np.float64)
    a, b, s = np.argwhere(fg), np.argwhere(~fg), np.asarray(sp, np.float64)
    if len(b) == 0:
        out[...] = np.inf
        return out
    if len(a) == 0:
        return out
    res = np.empty(len(a), np.float64)
    step = max(1, (1 << 21) // len(b))
    for i in range(0, len(a), step):
        t = (a[i:i + step, None, :] - b[None, :, :]).astype(np.float64) * s
        t = t * t
        res[i:i + step] = np.sqrt((t[..., 0] + (t[..., 1] + t[..., 2])).min(axis=1))
    out[fg] = res                                 # argwhere: raster order, as fg[...]
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------
class Case(object):
    def __init__(self, name, volume, classes=None):
        self.name, self.volume, self.classes = name, volume, classes


def _random(shape, seed, density=0.6):
    return (np.random.RandomState(seed).rand(*shape) < density).astype(np.int64)


def _bridge():
    v = np.zeros((6, 33, 18), np.int64)
    v[1:6, 2:12, 3:14] = 1
    v[1:6, 20:31, 3:14] = 1
    v[3, 12:20, 8] = 1                            # two blobs joined by a one-voxel bridge
    return v


def _on_face():
    v = np.zeros((5, 17, 33), np.int64)
    v[0:4, 0:9, 25:33] = 1                        # touches three faces
    v[2, 3, 28] = 0                               # and has a one-voxel gap
    return v


def _two_classes():
    v = np.zeros((4, 16, 16), np.int64)
    v[:, 2:7, 3:13] = 1
    v[:, 8:14, 3:13] = 2                          # one voxel (row 7) apart
    return v


def _classes(shape, seed, classes):
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, classes, tuple((s + 3) // 4 for s in shape))
    v = np.kron(coarse, np.ones((4, 4, 4), np.int64))[:shape[0], :shape[1], :shape[2]].copy()
    noise = rng.rand(*shape)
    v[noise < 0.25] = 0
    v[noise > 0.97] = classes + 2                 # out of range
    v[(noise > 0.94) & (noise <= 0.97)] = -1
    return v


@functools.lru_cache(maxsize=None)
def cases():
    """binary cases, then the class cases"""
    out = [Case('random %dx%dx%d' % s, _random(s, 100 + i)) for i, s in enumerate(SHAPES)]
    out += [Case('bridge', _bridge()), Case('on a face', _on_face()), Case('two classes as one', _two_classes())]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def class_cases():
    return (Case('two classes apart C3', _two_classes(), 3), Case('blocky C3', _classes((5, 17, 33), 7, 3), 3),
            Case('blocky C5', _classes((6, 33, 18), 8, 5), 5), Case('blocky C5 long', _classes((67, 3, 5), 9, 5), 5))


@functools.lru_cache(maxsize=None)
def reference(kind, index, op, setting):
    """the brute force of case `index` of cases() ('binary') or class_cases() ('classes'), computed once"""
    case = (cases() if kind == 'binary' else class_cases())[index]
    sp, r = SETTINGS[setting]
    out = brute(case.volume, op, r, sp, case.classes)
    out.setflags(write=False)
    return out
