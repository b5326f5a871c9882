"""Shared by test_postprocess_host.py and test_gpu_postprocess.py: small label volumes for the case post-processing
(aide_amd.inference.keep_components and fill_holes), chosen where the kernels can go wrong, and an independent statement of
both definitions: breadth-first search over face neighbours, no library call but numpy's zeros.  The device tile is
4 x 16 x 16 over the logical (i0, i1, i2): shapes sit below one tile, at exactly one tile, at odd sizes and over several tiles;
cavities and blobs cross tile borders; ties sit inside one tile and across tiles.

cases()            -> dict(holes=[HoleCase], components=[ComponentCase]); built once, volumes read-only
flood_components() -> (uint8 volume, int64 stats [C, 3])
flood_holes()      -> (uint8 volume, int64 stats [C, 2], dict(filled, mixed, open): the number of background blobs by fate)
holes_reference(), components_reference(): the flood fill of a case, computed once and shared by every test that needs it"""
from collections import deque, namedtuple

import numpy as np

SHAPES = ((1, 1, 1), (3, 3, 3), (4, 16, 16), (5, 17, 33), (9, 40, 21), (3, 1, 50), (6, 33, 18))
RANDOM_SHAPES = SHAPES[2:]                        # the five larger ones
AXES = (None, 2, 0)

# classes: None (binary) or C; axes: the slice axes the case is run under
HoleCase = namedtuple('HoleCase', 'name volume classes axes')
# top_k / min_voxels: as keep_components takes them
ComponentCase = namedtuple('ComponentCase', 'name volume classes top_k min_voxels')

_STEPS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def _blobs(vol, member, steps=_STEPS):
    """Blobs of the voxels with member(value), joined over `steps` where the values are EQUAL, in raster order of their first
    voxel: [(value, voxels, open, touched)] -- open: some step from the blob leaves the volume; touched: the set of the other
    values one step from it."""
    d0, d1, d2 = vol.shape
    val = vol.tolist()                            # nested lists in logical order, whatever the strides
    seen = np.zeros(vol.shape, bool)
    found = []
    for z in range(d0):
        for y in range(d1):
            for x in range(d2):
                v = val[z][y][x]
                if seen[z, y, x] or not member(v):
                    continue
                seen[z, y, x] = True
                todo, blob, is_open, touched = deque([(z, y, x)]), [], False, set()
                while todo:
                    a, b, e = todo.popleft()
                    blob.append((a, b, e))
                    for s0, s1, s2 in steps:
                        p, q, r = a + s0, b + s1, e + s2
                        if not (0 <= p < d0 and 0 <= q < d1 and 0 <= r < d2):
                            is_open = True
                        elif val[p][q][r] != v:
                            touched.add(val[p][q][r])
                        elif not seen[p, q, r]:
                            seen[p, q, r] = True
                            todo.append((p, q, r))
                found.append((v, blob, is_open, touched))
    return found


def _per_class(value, c):
    return list(value) if isinstance(value, (list, tuple)) else [value] * (c or 2)


def flood_components(vol, c, top_k=1, min_voxels=1):
    """c = None: one slot over all non-zero values, 1 written, nothing when no value is positive; c = C: one slot per class
    1 .. C - 1.  Per slot: larger blobs first, ties to the lower raster index of the first voxel; the first top_k (None: all)
    are kept, and of those the ones with at least min_voxels voxels.  stats row = (blobs, voxels, voxels kept)."""
    vol = np.asarray(vol)
    rows = c or 2
    ks, ms = _per_class(top_k, c), _per_class(min_voxels, c)
    out = np.zeros(vol.shape, np.uint8)
    stats = np.zeros((rows, 3), np.int64)
    if c is None and not (vol.size and vol.max() > 0):
        return out, stats
    d1, d2 = vol.shape[1:]
    slots = {}
    for v, blob, _, _ in _blobs(vol, (lambda v: v != 0) if c is None else (lambda v: 1 <= v < c)):
        z, y, x = blob[0]
        slots.setdefault(1 if c is None else v, []).append((-len(blob), (z * d1 + y) * d2 + x, blob))
    for cls, found in slots.items():
        found.sort(key=lambda f: f[:2])
        kept = [f for f in (found if ks[cls] is None else found[:ks[cls]]) if -f[0] >= ms[cls]]
        for _, _, blob in kept:
            for a, b, e in blob:
                out[a, b, e] = cls
        stats[cls] = len(found), -sum(f[0] for f in found), -sum(f[0] for f in kept)
    return out, stats


def flood_holes(vol, c, slice_axis=None):
    """Background: value 0.  A blob of background that no step leaves the volume from is a hole; steps along slice_axis do not
    exist.  c = None: a hole is filled with 1 and every non-zero value is written as 1.  c = C: a value 1 .. C - 1 is kept, any
    other written as 0, and a hole is filled with v when the values one step from it are {v} with 1 <= v < C."""
    vol = np.asarray(vol)
    rows = c or 2
    steps = tuple(s for s in _STEPS if slice_axis is None or s[slice_axis] == 0)
    if c is None:
        out = (vol != 0).astype(np.uint8)
    else:
        out = np.where((vol >= 1) & (vol < c), vol, 0).astype(np.uint8)
    stats = np.zeros((rows, 2), np.int64)
    fate = dict(filled=0, mixed=0, open=0)
    for _, blob, is_open, touched in _blobs(vol, lambda v: v == 0, steps):
        if is_open:
            fate['open'] += 1
            continue
        assert touched, 'a closed blob of background touches something'
        if c is None:
            fill = 1
        else:
            fill = next(iter(touched)) if len(touched) == 1 else 0
            fill = fill if 1 <= fill < c else 0
        if not fill:
            fate['mixed'] += 1
            continue
        fate['filled'] += 1
        stats[fill] += (1, len(blob))
        for a, b, e in blob:
            out[a, b, e] = fill
    return out, stats, fate


# ---- volumes ---------------------------------------------------------------------------------------------------------------
def serpentine(d0, d1, d2, value):
    """One component that winds through the whole volume: every other row of every other plane, rows joined at alternating
    ends, planes joined at one corner."""
    v = np.zeros((d0, d1, d2), np.int64)
    for z in range(0, d0, 2):
        for y in range(0, d1, 2):
            v[z, y, :] = value
            if y + 1 < d1:
                v[z, y + 1, d2 - 1 if (y // 2) % 2 == 0 else 0] = value
        if z + 1 < d0:
            v[z + 1, d1 - 1 if d1 % 2 == 1 else d1 - 2, 0] = value
    return v


def serpentine_case():
    """class 2 winds through every tile of (9, 33, 35); compact class-1 and class-3 blobs in the planes it leaves free"""
    v = serpentine(9, 33, 35, 2)
    v[1, 2:6, 5:9] = 1                            # 16 voxels
    v[3, 20:23, 14:18] = 1                        # 12, across the tile border at i2 = 16
    v[5, 10:13, 10:14] = 3                        # 12
    v[7, 15:17, 30:34] = 3                        # 8, across the borders at i1 = 16 and i2 = 32
    return v


def ties_case():
    """(9, 20, 40), C = 5.  Class 1: two blobs of 12 voxels in different tiles, A first in (i0, i1, i2) order, B first in
    (i2, i0, i1) order.  Class 3: two blobs of 3 voxels inside one tile.  Class 2: one blob of 12 voxels across the tile
    borders at i0 = 4 and i2 = 32.  Class 4: single voxels only (every one a tie)."""
    v = np.zeros((9, 20, 40), np.int64)
    v[0:2, 0:2, 20:23] = 1                        # A
    v[5:7, 17:19, 0:3] = 1                        # B
    v[0, 4, 17:20] = 3
    v[2, 8, 20:23] = 3
    v[3:5, 5:7, 30:33] = 2
    v[8, 0, 39] = 4
    v[8, 19, 0] = 4
    v[0, 19, 39] = 4
    return v


def adjacent_case():
    """two classes that meet at a tile border (i2 = 16) and a third that touches both inside the tiles: no merge"""
    v = np.zeros((5, 20, 40), np.int64)
    v[:, :, :16] = 1
    v[:, :, 16:] = 2
    v[1:4, 3:9, 10:22] = 3
    v[4, 19, 10] = 2                              # a class-2 voxel enclosed by class 1 and the walls: its own blob
    return v


def three_blobs():
    """(9, 20, 40), one value: blobs of 30, 18 (across the tile borders at i0 = 4 and i2 = 16) and 7 voxels, and one of 18 that
    comes later in raster order than the other of 18"""
    v = np.zeros((9, 20, 40), np.int64)
    v[0:2, 0:3, 0:5] = 1                          # 30
    v[3:6, 4:6, 15:18] = 1                        # 18, first voxel (3, 4, 15)
    v[8, 19, 33:40] = 1                           # 7
    v[6:8, 10:13, 30:33] = 1                      # 18, first voxel (6, 10, 30)
    return v


def shell(shape, lo, hi, value, inside=0):
    """a box of `value` with the cavity [lo, hi) of `inside`"""
    v = np.full(shape, value, np.int64)
    v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = inside
    return v


def _random(shape, density, classes, seed):
    rng = np.random.RandomState(seed)
    fg = rng.rand(*shape) < density
    return np.where(fg, rng.randint(1, classes, shape) if classes > 2 else 1, 0).astype(np.int64)


def _hole_cases():
    out = []
    for n, shape in enumerate(RANDOM_SHAPES):
        for density in (0.6, 0.8):
            tag = '%s %.1f' % ('x'.join(map(str, shape)), density)
            out.append(HoleCase('random binary ' + tag, _random(shape, density, 2, 300 + 10 * n + int(density * 10)), None, AXES))
            out.append(HoleCase('random classes ' + tag, _random(shape, density, 5, 400 + 10 * n + int(density * 10)), 5, AXES))
    for seed in (7, 8):
        rng = np.random.RandomState(seed)
        organs = np.kron(rng.randint(1, 4, (2, 5, 6)), np.ones((5, 8, 6), np.int64))     # blocks of classes 1 .. 3
        out.append(HoleCase('blocky %d' % seed, np.where(rng.rand(10, 40, 36) < 0.15, 0, organs).astype(np.int64), 5, AXES))
    centre = shell((3, 3, 3), (1, 1, 1), (2, 2, 2), 1)
    out.append(HoleCase('centre', centre, None, AXES))
    out.append(HoleCase('centre classes', 3 * centre, 5, AXES))
    across = shell((9, 40, 40), (2, 10, 12), (7, 20, 36), 2)      # crosses i0 = 4, i1 = 16, i2 = 16 and 32
    out.append(HoleCase('cavity across tiles', across, None, AXES))
    out.append(HoleCase('cavity across tiles classes', across, 4, AXES))
    channel = across.copy()
    channel[4, 15, 36:] = 0                       # one voxel wide, to the face i2 = 39
    out.append(HoleCase('channel', channel, None, AXES))
    out.append(HoleCase('channel classes', channel, 4, AXES))
    diagonal = np.ones((5, 6, 6), np.int64)
    diagonal[0, 0, 0] = 0                         # on three faces
    diagonal[1, 1, 1] = 0                         # meets it at a corner only
    diagonal[3, 4, 4] = 0
    diagonal[4, 5, 4] = 0                         # on a face, meets the voxel above along an edge only
    out.append(HoleCase('diagonal', diagonal, None, AXES))
    out.append(HoleCase('diagonal classes', diagonal, 2, AXES))
    island = shell((9, 20, 36), (2, 4, 10), (7, 18, 34), 2)
    island[4:6, 8:12, 15:20] = 2                  # floats in the cavity
    out.append(HoleCase('island same class', island, 5, AXES))
    other = island.copy()
    other[4:6, 8:12, 15:20] = 3
    out.append(HoleCase('island other class', other, 5, AXES))
    out.append(HoleCase('island other class binary', other, None, AXES))
    two = shell((6, 20, 20), (2, 5, 5), (4, 17, 17), 1)
    two[:, :, 10:] = np.where(two[:, :, 10:] == 1, 2, 0)
    out.append(HoleCase('two-class shell', two, 5, AXES))
    far = shell((6, 20, 20), (2, 5, 5), (4, 17, 17), 1)
    far[3, 4, 9] = 7                              # in the shell, one step from the cavity
    out.append(HoleCase('out of range neighbour', far, 5, AXES))
    out.append(HoleCase('out of range neighbour binary', far, None, AXES))
    neg = far.copy()
    neg[3, 4, 9] = -3
    out.append(HoleCase('negative neighbour', neg, 5, AXES))
    tube = np.ones((6, 8, 40), np.int64)
    tube[2:4, 3:5, :] = 0                         # open at both ends of axis 2, across the tile borders at i0 = 4, i2 = 16, 32
    out.append(HoleCase('tube', tube, None, AXES))
    out.append(HoleCase('tube classes', 2 * tube, 3, AXES))
    out.append(HoleCase('all zero', np.zeros((5, 17, 33), np.int64), None, AXES))
    out.append(HoleCase('all zero classes', np.zeros((5, 17, 33), np.int64), 5, AXES))
    out.append(HoleCase('all foreground', np.ones((5, 17, 33), np.int64), None, AXES))
    out.append(HoleCase('all foreground classes', np.full((5, 17, 33), 4, np.int64), 5, AXES))
    out.append(HoleCase('one voxel zero', np.zeros((1, 1, 1), np.int64), None, AXES))
    out.append(HoleCase('one voxel one', np.ones((1, 1, 1), np.int64), 2, AXES))
    blocky = [case.volume for case in out if case.name == 'blocky 7'][0]
    out.append(HoleCase('blocky permuted', blocky.transpose(2, 0, 1), 5, AXES))       # a view: logical (36, 10, 40)
    out.append(HoleCase('cavity permuted', across.transpose(1, 2, 0), None, AXES))
    rng = np.random.RandomState(11)
    bytes_ = np.where(rng.rand(6, 33, 18) < 0.75, np.array([1, 2, 3, 253], np.uint8)[rng.randint(0, 4, (6, 33, 18))], 0)
    out.append(HoleCase('uint8 classes', bytes_.astype(np.uint8), 4, AXES))
    out.append(HoleCase('uint8 binary', bytes_.astype(np.uint8), None, AXES))
    out.append(HoleCase('uint8 permuted', bytes_.astype(np.uint8).transpose(1, 2, 0), 4, AXES))
    return out


def _component_cases():
    out = []
    for n, shape in enumerate(RANDOM_SHAPES):
        for density in (0.6, 0.8):
            tag = '%s %.1f' % ('x'.join(map(str, shape)), density)
            out.append(ComponentCase('random binary ' + tag, _random(shape, density - 0.3, 2, 500 + 10 * n + int(density * 10)),
                                     None, 3, 2))
            out.append(ComponentCase('random classes ' + tag, _random(shape, density, 5, 600 + 10 * n + int(density * 10)), 5,
                                     (0, 1, 2, 8, None), (1, 1, 3, 2, 4)))
    for shape in SHAPES[:2]:
        out.append(ComponentCase('tiny %s' % 'x'.join(map(str, shape)), _random(shape, 0.5, 3, 3), 3, 2, 1))
    t = ties_case()
    out.append(ComponentCase('ties top 1', t, 5, 1, 1))
    out.append(ComponentCase('ties top 1 permuted', t.transpose(2, 0, 1), 5, 1, 1))      # a view: logical (40, 9, 20)
    out.append(ComponentCase('ties binary top 1', (t == 1).astype(np.int64), None, 1, 1))
    out.append(ComponentCase('ties binary top 1 permuted', (t == 1).astype(np.int64).transpose(2, 0, 1), None, 1, 1))
    out.append(ComponentCase('ties per class', t, 5, (0, 1, 2, 2, 1), 1))
    out.append(ComponentCase('ties per class floor', t, 5, (0, 2, 2, 2, None), (1, 12, 13, 3, 2)))
    out.append(ComponentCase('single voxels top 2', (t == 4).astype(np.int64), None, 2, 1))
    out.append(ComponentCase('single voxels top 2 permuted', (t == 4).astype(np.int64).transpose(2, 0, 1), None, 2, 1))
    b = three_blobs()
    out.append(ComponentCase('three blobs top 2', b, None, 2, 1))
    out.append(ComponentCase('three blobs top 3', b, None, 3, 1))
    out.append(ComponentCase('three blobs top 2 floor 19', b, None, 2, 19))              # the second is below the floor
    out.append(ComponentCase('three blobs top 3 classes', 2 * b, 3, 3, 1))
    for floor in (17, 18, 19):
        out.append(ComponentCase('three blobs all floor %d' % floor, b, None, None, floor))
    out.append(ComponentCase('three blobs floor above all', b, None, None, 31))
    out.append(ComponentCase('three blobs floor 2^40', b, 2, 8, 2 ** 40))
    out.append(ComponentCase('three blobs top 8', b, None, 8, 1))
    out.append(ComponentCase('serpentine', serpentine_case(), 5, 2, 9))
    out.append(ComponentCase('serpentine binary', serpentine_case(), None, 3, 1))
    out.append(ComponentCase('adjacent', adjacent_case(), 5, (0, 1, 1, 1, 1), (1, 1, 2, 1, 1)))
    out.append(ComponentCase('adjacent top 2', adjacent_case(), 4, 2, 1))
    rng = np.random.RandomState(5)
    wide = np.array([-3, 0, 1, 2, 3, 4, 5, 7])[rng.randint(0, 8, (9, 40, 21))].astype(np.int64)
    out.append(ComponentCase('out of range', wide, 5, 4, 2))
    out.append(ComponentCase('out of range binary', wide, None, 4, 2))
    out.append(ComponentCase('negative only', -np.ones((3, 5, 7), np.int64), None, 2, 1))
    out.append(ComponentCase('all zero', np.zeros((5, 17, 33), np.int64), 5, 2, 1))
    out.append(ComponentCase('eight classes', rng.randint(0, 8, (9, 40, 21)).astype(np.int64), 8, (0, 1, 2, 3, 4, 5, 6, 8), 2))
    return out


_CASES = {}
_REFERENCE = {}


def holes_reference(index, axis):
    """flood_holes of hole case `index` under slice axis `axis`, computed once"""
    key = ('holes', index, axis)
    if key not in _REFERENCE:
        case = cases()['holes'][index]
        out, stats, fate = flood_holes(case.volume, case.classes, axis)
        out.flags.writeable = stats.flags.writeable = False
        _REFERENCE[key] = out, stats, fate
    return _REFERENCE[key]


def components_reference(index):
    key = ('components', index)
    if key not in _REFERENCE:
        case = cases()['components'][index]
        out, stats = flood_components(case.volume, case.classes, case.top_k, case.min_voxels)
        out.flags.writeable = stats.flags.writeable = False
        _REFERENCE[key] = out, stats
    return _REFERENCE[key]


def cases():
    """The case lists, built once.  Every generated hole case is held to the properties it is there for, stated on the flood
    fill alone, so that no test can pass on inputs where nothing happens."""
    if _CASES:
        return _CASES
    _CASES.update(holes=_hole_cases(), components=_component_cases())
    for lst in _CASES.values():
        for case in lst:
            case.volume.flags.writeable = False
    for index, case in enumerate(_CASES['holes']):
        generated = case.name.startswith(('random', 'blocky'))
        if not generated:
            continue
        for axis in case.axes:
            fate = holes_reference(index, axis)[2]
            if 1 in case.volume.shape:            # (3, 1, 50): no hole is possible, in 3-D or in a slice that holds the thin axis
                thin = case.volume.shape.index(1)
                if axis is None or axis != thin:
                    assert fate['filled'] == 0 and fate['mixed'] == 0 and fate['open'] >= 1, (case.name, axis, fate)
                    continue
            assert fate['open'] >= 1, (case.name, axis, fate)
            assert fate['filled'] + fate['mixed'] >= 1, (case.name, axis, fate)
            if case.classes is None or case.name.startswith('blocky'):
                assert fate['filled'] >= 1, (case.name, axis, fate)
            if case.classes is not None:
                assert fate['mixed'] >= 1, (case.name, axis, fate)
    return _CASES
