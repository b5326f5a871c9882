"""Shared by test_surface_select_host.py and test_gpu_surface_select.py: what the percentiles (HD95) and the tolerance counts
(NSD) of aide_amd/utils/metrics3d.py must be, from np.sort of the reference distances of surface_cases.py.

Tolerances.  surface_cases.py derives that two implementations of the distance recipe differ by at most 2^-50 relative per
distance, and sets REL = 2^-49.  Perturbing every value of a multiset by a relative eps moves every order statistic by at most
eps (the k-th smallest of the perturbed values lies between the perturbed k-th smallest from below and from above), so x[lo]
and x[hi] carry the bound of a single distance.  value = x[lo] + (x[hi] - x[lo]) * f with 0 <= f < 1 and x[lo] * (1 - f),
x[hi] * f <= value moves by at most eps * value, plus three roundings of quantities no larger than value (3 * 2^-53): below
2^-50 + 2^-51 < REL.  With spacing (1, 1, 1) every distance is bit-equal, hence every order statistic and, the formula being
the same float64 operations on both sides, every percentile: same_float.  Counts are integers and exact, which needs a
tolerance that no distance comes close to: at unit spacing values that ARE attained (1, 2, sqrt 2: `<=` against `<`), where
distances are bit-equal; otherwise midpoints between two neighbouring distinct reference distances, with the condition (on the
case, asserted by taus_for) that no reference distance lies within 2 * REL * tau of tau."""
import math

import numpy as np

from surface_cases import (REL, SMALL_SHAPES, SPACINGS, brute, class_pair, close, corner_blobs, ellipsoid_pair,  # noqa: F401
                           random_pair, reference, same_float)

UNIT = (1.0, 1.0, 1.0)
UNIT_TAUS = (1.0, 2.0, float(np.sqrt(2.0)))
QS = ((0.0, 25.0, 50.0, 95.0), (100.0,))
# random_pair(shape, 0.3, seed) per SMALL_SHAPES entry: seeds for which both borders have at least three voxels and taus_for's
# condition holds at every entry of SPACINGS (searched on the CPU from 300 upwards; (1, 7, 1) needs 322)
SMALL_SEEDS = (300, 322, 300, 300)


def small_cases():
    for shape, seed in zip(SMALL_SHAPES, SMALL_SEEDS):
        yield (shape,) + random_pair(shape, 0.3, seed)


def lists(ref):
    """-> sorted A, B and A+B from a reference dict of surface_cases"""
    a, b = (np.sort(ref[k][ref[k] >= 0]) for k in ('dist_P', 'dist_T'))
    return a, b, np.sort(np.concatenate([a, b]))


def rank_of(m, q):
    pos = (m - 1) * float(q) / 100.0
    lo = int(math.floor(pos))
    return pos, lo, min(lo + 1, m - 1)


def percentile(x, q):
    """x ascending, len >= 1 -> the percentile by the definition"""
    pos, lo, hi = rank_of(len(x), q)
    return np.float64(x[lo] + (x[hi] - x[lo]) * (pos - lo))


def expected(ref, qs, taus):
    """the entries surface_scores adds (binary mode) from the reference distances"""
    a, b, ab = lists(ref)
    empty = ref['n_P'] == 0 or ref['n_T'] == 0
    nan = np.full(len(qs), np.nan)
    e = dict(HD_pred=nan, HD_target=nan, HD=nan, HD_pooled=nan)
    if not empty:
        assert len(a) == ref['n_P'] and len(b) == ref['n_T']
        e = dict(HD_pred=np.array([percentile(a, q) for q in qs]), HD_target=np.array([percentile(b, q) for q in qs]),
                 HD_pooled=np.array([percentile(ab, q) for q in qs]))
        e['HD'] = np.maximum(e['HD_pred'], e['HD_target'])
    wp = np.array([0 if empty else np.count_nonzero(a <= t) for t in taus], np.int64)
    wt = np.array([0 if empty else np.count_nonzero(b <= t) for t in taus], np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        nsd = np.full(len(taus), np.nan) if empty else (wp + wt).astype(np.float64) / np.float64(ref['n_P'] + ref['n_T'])
    e.update(n_pred_within=wp, n_target_within=wt, NSD=nsd)
    return e


def taus_for(ref, spacing, count=2):
    """tolerances for a case: attained values at unit spacing, otherwise `count` midpoints between neighbouring distinct
    reference distances, none of which has a reference distance within 2 * REL * tau"""
    if tuple(spacing) == UNIT:
        return UNIT_TAUS
    ab = np.unique(lists(ref)[2])
    assert len(ab) >= 2, 'the case has fewer than two distinct distances: choose another'
    taus = []
    for k in range(count):
        i = min(len(ab) - 2, (k + 1) * (len(ab) - 1) // (count + 1))
        tau = 0.5 * (ab[i] + ab[i + 1])
        assert ab[i] < tau < ab[i + 1] and np.all(np.abs(ab - tau) > 2.0 * REL * tau), ('tau too close to a distance', tau)
        taus.append(float(tau))
    return tuple(taus)


def check_select(got, ref, spacing, qs, taus, what=''):
    """the percentile / tolerance entries of a surface_scores dict (binary mode) against the reference"""
    unit = tuple(spacing) == UNIT
    e = expected(ref, qs, taus)
    if qs:
        assert np.array_equal(got['percentiles'], np.array(qs, np.float64))
        for k in ('HD_pred', 'HD_target', 'HD', 'HD_pooled'):
            g = np.asarray(got[k])
            assert g.shape == (len(qs),) and g.dtype == np.float64, (what, k, g.shape, g.dtype)
            for j in range(len(qs)):
                ok = same_float(g[j], e[k][j]) if unit else close(g[j], e[k][j], REL)
                assert ok, (what, k, qs[j], float(g[j]), float(e[k][j]))
    if taus:
        assert np.array_equal(got['tolerances'], np.array(taus, np.float64))
        for k in ('n_pred_within', 'n_target_within'):
            g = np.asarray(got[k])
            assert g.shape == (len(taus),) and g.dtype == np.int64 and np.array_equal(g, e[k]), (what, k, g, e[k])
        g = np.asarray(got['NSD'])
        assert g.shape == (len(taus),) and all(same_float(x, y) for x, y in zip(g, e['NSD'])), (what, 'NSD', g, e['NSD'])
