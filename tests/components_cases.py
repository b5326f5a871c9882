"""Shared by test_components_host.py and test_gpu_components.py: the cases of the labelled components and the lesion-wise
counts (aide_amd.inference.label_components, lesion_counts, lesion_scores) and an independent statement of both definitions on
the breadth-first search of postprocess_cases (`_blobs`: no library call but numpy's zeros; it returns the blobs in raster order
of their first voxel, which is the numbering).  The device tile is 4 x 16 x 16 over the logical (i0, i1, i2).

label_cases() -> [LabelCase]: every distinct volume of postprocess_cases.cases()['components'] in binary form and with C = 5 or
                 the case's own C, and uint8 / int32 inputs
pair_cases()  -> [PairCase]: hand-built and random (pred, target) pairs
flood_labels(), flood_pair() + flood_lesions(): the flood fill; label_reference(), pair_reference(): computed once and shared"""
from collections import namedtuple

import numpy as np

import postprocess_cases as pc
from postprocess_cases import _blobs, _random, serpentine_case, ties_case, adjacent_case, three_blobs, SHAPES, RANDOM_SHAPES

LabelCase = namedtuple('LabelCase', 'name volume classes')
PairCase = namedtuple('PairCase', 'name pred target classes')
OVERLAPS = (0.0, 0.1, 0.5, 1.0)
PAIR_SHAPE = (9, 20, 40)


def _member(c):
    return (lambda v: v != 0) if c is None else (lambda v: 1 <= v < c)


def flood_labels(vol, c, cap=65536):
    """-> (labels int32, number of blobs, props int64 [cap, 12]); row j - 1 of props describes blob j as (value, area, first
    raster index, min0, min1, min2, max0 + 1, max1 + 1, max2 + 1, sum i0, sum i1, sum i2), rows past the blobs are zero"""
    vol = np.asarray(vol)
    d1, d2 = vol.shape[1:]
    labels = np.zeros(vol.shape, np.int32)
    props = np.zeros((cap, 12), np.int64)
    blobs = _blobs(vol, _member(c)) if vol.size else []
    for j, (v, blob, _, _) in enumerate(blobs):
        for a, b, e in blob:
            labels[a, b, e] = j + 1
        if j < cap:
            z, y, x = blob[0]
            cols = list(zip(*blob))
            props[j] = ([v, len(blob), (z * d1 + y) * d2 + x] + [min(col) for col in cols] + [max(col) + 1 for col in cols] +
                        [sum(col) for col in cols])
    return labels, len(blobs), props


def flood_pair(pred, target, c):
    """per side (0: the blobs of target, 1: the blobs of pred), in raster order: [(row of the table, area, cover)] with cover = the
    voxels of the blob at which the other volume is not 0 (c = None) or holds the blob's value (c = C)"""
    sides = []
    for a, b in ((target, pred), (pred, target)):
        other = np.asarray(b).tolist()
        found = []
        for v, blob, _, _ in _blobs(np.asarray(a), _member(c)):
            if c is None:
                cover = sum(1 for z, y, x in blob if other[z][y][x] != 0)
            else:
                cover = sum(1 for z, y, x in blob if other[z][y][x] == v)
            found.append((1 if c is None else v, len(blob), cover))
        sides.append(found)
    return sides


def counts(area, cover, overlap):
    """the rule: at least one voxel, and one float64 multiply and one compare"""
    return cover >= 1 and float(cover) >= overlap * float(area)


def flood_lesions(sides, c, overlap):
    """int64 [C or 2, 6]: target blobs, target blobs that count, pred blobs, pred blobs that count, sum of cover over the target
    blobs, pred voxels in blobs that do not count"""
    out = np.zeros((c or 2, 6), np.int64)
    for side, found in enumerate(sides):
        for row, area, cover in found:
            hit = counts(area, cover, overlap)
            out[row, 2 * side] += 1
            out[row, 2 * side + 1] += hit
            if side == 0:
                out[row, 4] += cover
            elif not hit:
                out[row, 5] += area
    return out


def scores_of(table, c):
    """the dict of lesion_scores from a table, stated again: scalars in the binary form, [C] arrays with classes"""
    rows = table[1] if c is None else table
    names = ('target_blobs', 'detected', 'pred_blobs', 'matched', 'covered_voxels', 'spurious_voxels')
    res = {name: (int(rows[k]) if c is None else rows[:, k].copy()) for k, name in enumerate(names)}
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.asarray(rows[..., 1], np.float64) / np.asarray(rows[..., 0], np.float64)
        p = np.asarray(rows[..., 3], np.float64) / np.asarray(rows[..., 2], np.float64)
        res.update(sensitivity=s, precision=p, F1=2 * s * p / (s + p))
    return res


# ---- label cases -----------------------------------------------------------------------------------------------------------
def _label_cases():
    out, seen = [], set()
    for case in pc.cases()['components']:
        vol = case.volume
        key = (vol.tobytes(), vol.shape, vol.strides)
        if key in seen:
            continue
        seen.add(key)
        name = case.name + ' ' + 'x'.join(map(str, vol.shape))
        out.append(LabelCase(name + ' binary', vol, None))
        out.append(LabelCase(name + ' C=%d' % (case.classes or 5), vol, case.classes or 5))
    assert len(seen) >= 30
    t = ties_case()
    out.append(LabelCase('ties uint8 C=5', t.astype(np.uint8), 5))
    out.append(LabelCase('ties uint8 permuted binary', t.astype(np.uint8).transpose(2, 0, 1), None))
    out.append(LabelCase('serpentine int32 C=4', serpentine_case().astype(np.int32), 4))
    out.append(LabelCase('serpentine int32 binary', serpentine_case().astype(np.int32), None))
    wide = [case.volume for case in pc.cases()['components'] if case.name == 'out of range'][0]
    out.append(LabelCase('out of range int32 C=3', wide.astype(np.int32), 3))
    out.append(LabelCase('adjacent uint8 C=2', adjacent_case().astype(np.uint8), 2))
    out.append(LabelCase('three blobs int32 permuted C=2', three_blobs().astype(np.int32).transpose(1, 2, 0), 2))
    return out


# ---- pair cases ------------------------------------------------------------------------------------------------------------
def hand_pair():
    """(pred, target) on (9, 20, 40), C = 5; see HAND for what every blob is there for"""
    t = np.zeros(PAIR_SHAPE, np.int64)
    p = np.zeros(PAIR_SHAPE, np.int64)
    t[0:2, 0:2, 0:3] = 1                          # fully covered: 12 of 12
    p[0:2, 0:2, 0:3] = 1
    t[0:2, 6:8, 0:3] = 1                          # half covered: 6 of 12, overlap = 0.5 sits on the threshold
    p[0:1, 6:8, 0:3] = 1
    t[0:2, 12:14, 0:3] = 2                        # touched by a single voxel of a pred blob of two
    p[1, 13:15, 2] = 2
    t[6:8, 0:2, 0:3] = 3                          # missed
    p[6:8, 6:8, 0:3] = 3                          # spurious
    t[0, 0:2, 20:22] = 1                          # two target blobs of 4 ...
    t[0, 0:2, 24:26] = 1
    p[0, 0:2, 20:26] = 1                          # ... bridged by one pred blob of 12
    t[3:5, 10:12, 14:34] = 2                      # one target blob of 80 across the tile borders at i0 = 4 and i2 = 16, 32 ...
    p[3:5, 10:12, 14:22] = 2                      # ... split into two pred blobs of 32, one across i2 = 16,
    p[3:5, 10:12, 26:34] = 2                      # one across i2 = 32, both across i0 = 4
    t[6:8, 12:14, 20:23] = 4                      # a pred blob of the wrong class on top of a target blob:
    p[6:8, 12:14, 20:23] = 3                      # counts in the binary form and not with classes
    return p, t


# (target blobs, detected, pred blobs, matched) summed over the classes, by (classes, overlap): worked out by hand from the
# comments of hand_pair.  Target blobs: covered 12/12, half 6/12, touched 1/12, missed 0/12, two bridged 4/4, split 64/80, wrong
# class 0/12 (binary 12/12).  Pred blobs: 12/12, 6/6, 1/2, spurious 0/12, bridge 8/12, two halves 32/32, wrong class 0/12 (12/12)
HAND = {
    (5, 0.0): (8, 6, 8, 6), (5, 0.1): (8, 5, 8, 6), (5, 0.5): (8, 5, 8, 6), (5, 1.0): (8, 3, 8, 4),
    (None, 0.0): (8, 7, 8, 7), (None, 0.1): (8, 6, 8, 7), (None, 0.5): (8, 6, 8, 7), (None, 1.0): (8, 4, 8, 5),
}


def _redrawn(target, density, classes, seed):
    """target with about 15 % of its voxels drawn again"""
    rng = np.random.RandomState(seed)
    again = rng.rand(*target.shape) < 0.15
    return np.where(again, _random(target.shape, density, classes, seed + 1), target).astype(np.int64)


def _pair_cases():
    out = []
    p, t = hand_pair()
    out.append(PairCase('hand C=5', p, t, 5))
    out.append(PairCase('hand binary', p, t, None))
    out.append(PairCase('hand C=5 swapped', t, p, 5))
    out.append(PairCase('hand binary swapped', t, p, None))
    out.append(PairCase('hand C=4: class 4 is no member', p, t, 4))
    for n, shape in enumerate(RANDOM_SHAPES):
        for density in (0.6, 0.8):
            tag = '%s %.1f' % ('x'.join(map(str, shape)), density)
            seed = 700 + 10 * n + int(density * 10)
            t = _random(shape, density - 0.45, 2, seed)
            out.append(PairCase('random binary ' + tag, _redrawn(t, density - 0.45, 2, seed + 100), t, None))
            t = _random(shape, density, 5, seed + 200)
            out.append(PairCase('random classes ' + tag, _redrawn(t, density, 5, seed + 300), t, 5))
    names = {case.name: case for case in out}
    base = names['random classes 9x40x21 0.6']
    out.append(PairCase('random classes swapped', base.target, base.pred, 5))
    view = np.ascontiguousarray(base.pred.transpose(1, 2, 0)).transpose(2, 0, 1)          # a view: logical (9, 40, 21)
    assert view.shape == base.pred.shape and not view.flags['C_CONTIGUOUS'] and np.array_equal(view, base.pred)
    out.append(PairCase('random classes permuted pred', view, base.target, 5))
    base = names['random binary 6x33x18 0.8']
    view = np.ascontiguousarray(base.pred.transpose(2, 0, 1)).transpose(1, 2, 0)
    out.append(PairCase('random binary permuted pred', view, base.target, None))
    out.append(PairCase('random binary uint8 pred int32 target', base.pred.astype(np.uint8), base.target.astype(np.int32), None))
    base = names['random classes 5x17x33 0.8']
    out.append(PairCase('random classes uint8 pred int32 target', base.pred.astype(np.uint8), base.target.astype(np.int32), 5))
    wide = [case.volume for case in pc.cases()['components'] if case.name == 'out of range'][0]
    out.append(PairCase('out of range C=5', _redrawn(wide, 0.6, 5, 41), wide, 5))
    out.append(PairCase('out of range binary', _redrawn(wide, 0.6, 5, 41), wide, None))
    p, t = hand_pair()
    zero = np.zeros(PAIR_SHAPE, np.int64)
    for c in (None, 5):
        tag = 'binary' if c is None else 'C=5'
        out.append(PairCase('all-zero pred ' + tag, zero, t, c))
        out.append(PairCase('all-zero target ' + tag, p, zero, c))
        out.append(PairCase('both all-zero ' + tag, zero, zero, c))
    return out


_CASES = {}
_REFERENCE = {}


def label_cases():
    if 'labels' not in _CASES:
        _CASES['labels'] = _label_cases()
    return _CASES['labels']


def pair_cases():
    """The pair cases, built once.  Every generated pair is held to the condition it is there for, stated on the flood fill alone:
    at overlap = 0.5 each side has at least one blob that counts and at least one that does not.  The hand pair is held to HAND."""
    if 'pairs' in _CASES:
        return _CASES['pairs']
    _CASES['pairs'] = _pair_cases()
    for case in _CASES['pairs']:
        case.pred.flags.writeable = case.target.flags.writeable = False
    for index, case in enumerate(_CASES['pairs']):
        if case.name.startswith(('random', 'out of range')):
            for side, found in enumerate(pair_reference(index)):
                hits = [counts(area, cover, 0.5) for _, area, cover in found]
                assert any(hits) and not all(hits), (case.name, side, len(hits), sum(hits))
        if case.name in ('hand C=5', 'hand binary'):
            for overlap in OVERLAPS:
                table = flood_lesions(pair_reference(index), case.classes, overlap)
                assert tuple(table[:, :4].sum(axis=0)) == HAND[(case.classes, overlap)], (case.name, overlap, table)
    return _CASES['pairs']


def label_reference(index):
    """flood_labels of label case `index` at the default cap, computed once"""
    key = ('labels', index)
    if key not in _REFERENCE:
        case = label_cases()[index]
        labels, count, props = flood_labels(case.volume, case.classes)
        labels.flags.writeable = props.flags.writeable = False
        _REFERENCE[key] = labels, count, props
    return _REFERENCE[key]


def pair_reference(index):
    """flood_pair of pair case `index`, computed once: flood_lesions turns it into the table of any overlap"""
    key = ('pairs', index)
    if key not in _REFERENCE:
        case = _CASES['pairs'][index]
        _REFERENCE[key] = flood_pair(case.pred, case.target, case.classes)
    return _REFERENCE[key]


def lattice_case():
    """(34, 250, 250), not a multiple of the tile: single voxels of classes 1, 3, 4 on the [::2, ::2, ::2] lattice (265 625
    blobs: above the default cap of 65 536 and above 2^16) and one serpentine of class 2 that winds through the odd rows of
    the odd planes, which the lattice leaves free: 265 626 blobs.  Too large for the pure-Python flood fill: it is checked
    against the host statement, which the host tests hold to the flood fill on every small case."""
    d0, d1, d2 = 34, 250, 250
    v = np.zeros((d0, d1, d2), np.int64)
    rng = np.random.RandomState(9)
    v[::2, ::2, ::2] = np.array([1, 3, 4])[rng.randint(0, 3, (17, 125, 125))]
    for z in range(1, d0, 2):
        for y in range(1, d1, 2):
            v[z, y, :] = 2
            if y + 2 < d1:
                v[z, y + 1, d2 - 1 if (y // 2) % 2 == 0 else 0] = 2
        if z + 2 < d0:
            v[z + 1, 1, 1] = 2                    # odd i1 and i2: no lattice point
    return v
