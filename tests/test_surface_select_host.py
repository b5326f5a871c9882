"""Host side of the surface-distance percentiles (HD95) and tolerance counts (NSD) of aide_amd/utils/metrics3d.py: the host
path against an O(n^2) numpy evaluation and against np.percentile, the numpy model of the device's radix select against
np.sort, the C ABI of aide_surface3d_scores_select and its argument checks, the key sets and the Python errors.  No device."""
import ctypes

import numpy as np
import pytest
import torch

import surface_select_cases as ss


@pytest.fixture(scope='module')
def built():
    from aide_amd.build import build
    return build(verbose=False)


@pytest.mark.parametrize('spacing', ss.SPACINGS)
def test_host_path_equals_brute(spacing):
    from aide_amd.utils.metrics3d import surface_scores
    for shape, p, t in ss.small_cases():
        ref = ss.brute(p, t, spacing)
        assert ref['n_P'] >= 3 and ref['n_T'] >= 3
        taus = ss.taus_for(ref, spacing)
        for qs in ss.QS:
            got = surface_scores(p, t, spacing, percentiles=qs, tolerances=taus)
            ss.check_select(got, ref, spacing, qs, taus, (shape, spacing, qs))
        only_q = surface_scores(p, t, spacing, percentiles=(95,))
        assert 'NSD' not in only_q and 'tolerances' not in only_q and only_q['HD'].shape == (1,)
        only_t = surface_scores(torch.from_numpy(p), torch.from_numpy(t), spacing, tolerances=taus[:1])    # CPU tensors
        assert 'HD' not in only_t and 'percentiles' not in only_t
        ss.check_select(only_t, ref, spacing, (), taus[:1], 'tolerances only')


def test_against_numpy_percentile():
    """np.percentile's 'linear' method differs only in how pos rounds: pos moves by at most 8 m 2^-52, which crosses at most one
    order statistic, so the values differ by at most the spread of the neighbouring order statistics times that."""
    from aide_amd.utils.metrics3d import surface_scores
    for k, (shape, spacing) in enumerate(zip(ss.SMALL_SHAPES, ss.SPACINGS + ss.SPACINGS[:1])):
        p, t = ss.random_pair(shape, 0.3, seed=40 + k)
        qs = (0.0, 12.5, 33.3, 95.0)
        got = surface_scores(p, t, spacing, percentiles=qs)
        for key, x in zip(('HD_pred', 'HD_target', 'HD_pooled'), ss.lists(ss.reference(p, t, spacing))):
            m = len(x)
            for j, q in enumerate(qs):
                lo = ss.rank_of(m, q)[1]
                want = np.percentile(x, q)
                bound = (x[min(lo + 1, m - 1)] - x[max(lo - 1, 0)]) * 8 * m * 2.0 ** -52 + ss.REL * abs(want)
                assert abs(got[key][j] - want) <= bound, (shape, key, q, got[key][j], want)


def test_hand_cases_and_empty_rules():
    from aide_amd.utils.metrics3d import surface_scores, HD95_fn, NSD3d_fn
    from aide_amd.utils import HD95_fn as exported                        # noqa: F401
    p, t = np.zeros((6, 7, 5), np.int64), np.zeros((6, 7, 5), np.int64)
    p[1, 2, 3] = 1
    t[3, 5, 4] = 1
    d = float(np.sqrt(46.0))                                               # (0.5 * 2)^2 + (2 * 3)^2 + (3 * 1)^2
    s = surface_scores(p, t, (0.5, 2, 3), percentiles=(0, 50, 100), tolerances=(d, 6.0))
    for k in ('HD', 'HD_pred', 'HD_target', 'HD_pooled'):
        assert np.all(s[k] == d), k                                        # m = 1 per direction, m = 2 pooled
    assert list(s['n_pred_within']) == [1, 0] and list(s['NSD']) == [1.0, 0.0]
    assert HD95_fn(p, t, (0.5, 2, 3)) == d and HD95_fn(p, t, (0.5, 2, 3), pooled=True) == d
    assert NSD3d_fn(p, t, 7.0, (0.5, 2, 3)) == 1.0
    # three distances 0, 1, 3 against one voxel: percentile 50 = 1, 75 = 1 + (3 - 1) * 0.5, pooled of {0, 1, 3, 0}: 25 -> 0
    p = np.zeros((1, 1, 8), np.int64)
    p[0, 0, [2, 3, 5]] = 1
    t = np.zeros((1, 1, 8), np.int64)
    t[0, 0, 2] = 1
    s = surface_scores(p, t, (1, 1, 1), percentiles=(50, 75, 25), tolerances=(1.0,))
    assert list(s['HD_pred']) == [1.0, 2.0, 0.5] and list(s['HD_target']) == [0.0, 0.0, 0.0]
    assert list(s['HD']) == [1.0, 2.0, 0.5] and list(s['HD_pooled']) == [0.5, 1.5, 0.0]
    assert s['n_pred_within'][0] == 2 and s['n_target_within'][0] == 1 and s['NSD'][0] == 0.75
    # identical volumes
    e, _ = ss.ellipsoid_pair((12, 14, 9))
    s = surface_scores(e, e.copy(), (0.7, 0.7, 5.5), percentiles=(0, 95, 100), tolerances=(0.0,))
    assert np.all(s['HD'] == 0.0) and np.all(s['HD_pooled'] == 0.0) and s['NSD'][0] == 1.0
    # empty borders
    z, one = np.zeros((3, 4, 5), np.int64), np.zeros((3, 4, 5), np.int64)
    one[1, 1:3, 2] = 1
    for a, b in ((z, one), (one, z), (z, z)):
        s = surface_scores(a, b, (1, 2, 3), percentiles=(95,), tolerances=(1.0, 5.0))
        for k in ('HD', 'HD_pred', 'HD_target', 'HD_pooled'):
            assert s[k].shape == (1,) and np.isnan(s[k][0])
        assert np.all(np.isnan(s['NSD'])) and not s['n_pred_within'].any() and not s['n_target_within'].any()
        assert np.isnan(HD95_fn(a, b)) and np.isnan(NSD3d_fn(a, b, 1.0))


def test_classes_on_host():
    from aide_amd.inference import case_scores
    from aide_amd.utils.metrics3d import surface_scores
    sp = (0.7, 0.7, 5.5)
    p, t = ss.class_pair((9, 12, 7), seed=4)
    qs = (50.0, 95.0)
    taus = ss.taus_for(ss.brute(p, t, sp, cls=1), sp, count=1)
    s = surface_scores(p, t, sp, num_classes=5, percentiles=qs, tolerances=taus)
    assert s['percentiles'].shape == (2,) and s['tolerances'].shape == (1,)
    for k in ('HD', 'HD_pred', 'HD_target', 'HD_pooled'):
        assert s[k].shape == (5, 2) and s[k].dtype == np.float64 and np.all(np.isnan(s[k][0])) and np.all(np.isnan(s[k][3]))
    assert s['NSD'].shape == (5, 1) and np.isnan(s['NSD'][0, 0]) and np.isnan(s['NSD'][3, 0])
    for k in ('n_pred_within', 'n_target_within'):
        assert s[k].shape == (5, 1) and s[k].dtype == np.int64 and s[k][0, 0] == 0 and s[k][3, 0] == 0
    for c in (1, 2, 4):
        ref = ss.brute(p, t, sp, cls=c)
        e = ss.expected(ref, qs, taus)
        for k in ('HD', 'HD_pred', 'HD_target', 'HD_pooled'):
            assert all(ss.close(s[k][c, j], e[k][j], ss.REL) for j in range(2)), (c, k)
        # (tau was built for class 1: the counts of the other classes are compared where no distance is near it)
        if c == 1:
            assert s['n_pred_within'][c, 0] == e['n_pred_within'][0] and ss.same_float(s['NSD'][c, 0], e['NSD'][0])
    cs = case_scores(p, t, num_classes=5, spacing=sp, percentiles=qs, tolerances=taus)
    assert sorted(cs) == ['ASSD', 'Dice', 'FN', 'FP', 'HD', 'HD_pooled', 'IoU', 'MSSD', 'NSD', 'RAVD', 'TN', 'TP']
    for k in ('HD', 'HD_pooled', 'NSD'):
        assert np.array_equal(cs[k], s[k], equal_nan=True)


@pytest.mark.parametrize('m', [1, 2, 255, 256, 257, 70000])
def test_select_model_equals_sort(m):
    from aide_amd.utils.metrics3d import select_model
    rng = np.random.RandomState(m)
    pool = rng.randint(0, 2 ** 63, size=max(1, m // 40), dtype=np.int64).astype(np.uint64)
    pool[::2] |= np.uint64(1) << np.uint64(63)                              # both halves of the top digit
    keys = pool[rng.randint(0, len(pool), m)]
    if m >= 255:                                                            # a run that differs only in the last digit, and
        keys[:100] = (pool[0] & ~np.uint64(255)) | rng.randint(0, 3, 100).astype(np.uint64)
        keys[100:180] = np.sqrt(rng.randint(1, 6, 80)).view(np.uint64)     # bit patterns of attained distances
    want = np.sort(keys)
    runs = np.flatnonzero(want[1:] == want[:-1])                            # ranks inside runs of equal keys
    ranks = sorted(set([0, m - 1, m // 2] + [int(r) for r in runs[:: max(1, len(runs) // 6)]] + [int(r) + 1 for r in runs[-1:]]))
    got = select_model(keys, ranks)
    assert got.dtype == np.uint64 and np.array_equal(got, want[ranks]), (m, ranks)
    with pytest.raises(ValueError):
        select_model(keys, [m])


def test_select_model_on_distances():
    """keys = the bit patterns of non-negative doubles: the key order is the value order"""
    from aide_amd.utils.metrics3d import select_model
    p, t = ss.random_pair((17, 31, 16), 0.3, seed=9)
    for sp in ((1.0, 1.0, 1.0), (1.37, 1.37, 7.7)):
        a, b, ab = ss.lists(ss.reference(p, t, sp))
        for x in (a, b, ab):
            ranks = [0, len(x) // 4, ss.rank_of(len(x), 95.0)[1], len(x) - 1]
            got = select_model(np.random.RandomState(1).permutation(x).view(np.uint64), ranks)
            assert np.array_equal(got.view(np.float64), x[ranks])


def test_entry_point_abi_and_rejects_without_launch(built):
    """Answered on the host, before any HIP call (no device here)."""
    from aide_amd._lib import lib, parse_header
    protos = parse_header()
    assert len(protos['aide_surface3d_scores'][1]) == 21 and len(protos['aide_surface3d_ws_bytes'][1]) == 1    # unchanged
    assert len(protos['aide_surface3d_scores_select'][1]) == 25 and len(protos['aide_surface3d_select_ws_bytes'][1]) == 1
    assert protos['aide_surface3d_scores_select'][1][:17] == protos['aide_surface3d_scores'][1][:17]
    assert protos['aide_surface3d_select_ws_bytes'][0] is ctypes.c_size_t
    assert lib.aide_surface3d_select_ws_bytes(2 ** 31) == 0 and lib.aide_surface3d_select_ws_bytes(-1) == 0
    for n in (0, 1, 1000, 512 * 512 * 100, 2 ** 31 - 1):
        old, new = lib.aide_surface3d_ws_bytes(n), lib.aide_surface3d_select_ws_bytes(n)
        assert old + 16 * n <= new <= old + 16 * n + 65536 and new % 16 == 0, n
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    a += a % 16                                                             # 16-byte aligned inside buf
    good = (ctypes.c_double * 4)(0.0, 50.0, 95.0, 100.0)
    ok = dict(p=a, t=a, dims=(2, 2, 2), sp=(1.0, 1.0, 1.0), out=a, ws=a, q=good, nq=4, tol=good, nt=4)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.aide_surface3d_scores_select(v['p'], 0, 4, 2, 1, v['t'], 0, 4, 2, 1, *v['dims'], *v['sp'], -1, v['q'], v['nq'],
                                                v['tol'], v['nt'], v['out'], None, v['ws'], None)

    def arr(*v):
        return (ctypes.c_double * len(v))(*v)
    old_rejects = (dict(p=None), dict(t=None), dict(out=None), dict(ws=None), dict(ws=a + 8), dict(dims=(2 ** 16, 2 ** 15, 1)),
                   dict(dims=(-1, 2, 2)), dict(sp=(0.0, 1.0, 1.0)), dict(sp=(1.0, -1.0, 1.0)), dict(sp=(1.0, 1.0, float('nan'))),
                   dict(sp=(float('inf'), 1.0, 1.0)))
    new_rejects = (dict(nq=5), dict(nq=-1), dict(nt=5), dict(nt=-1), dict(q=None), dict(tol=None), dict(q=None, nq=1),
                   dict(tol=None, nt=1), dict(q=arr(-0.5), nq=1), dict(q=arr(50.0, 100.5), nq=2), dict(q=arr(float('nan')), nq=1),
                   dict(q=arr(float('inf')), nq=1), dict(tol=arr(-1.0), nt=1), dict(tol=arr(1.0, float('nan')), nt=2),
                   dict(tol=arr(float('inf')), nt=1), dict(tol=arr(0.0, 1.0, 2.0, -1e-300), nt=4))
    for kw in old_rejects + new_rejects:
        assert call(**kw) < 0, kw
    # the old entry's rejections also hold with nothing asked for
    for kw in old_rejects:
        assert call(q=None, nq=0, tol=None, nt=0, **kw) < 0, kw


def test_default_key_sets_are_unchanged():
    from aide_amd.inference import case_scores
    from aide_amd.utils.metrics3d import surface_scores
    p, t = ss.random_pair((6, 9, 5), 0.4, seed=8)
    sp = (1.4, 1.4, 7.0)
    base = ['ASSD', 'MSSD', 'RAVD', 'V_pred', 'V_target', 'n_pred', 'n_target']
    assert sorted(surface_scores(p, t, sp)) == base
    assert sorted(surface_scores(p, t, sp, num_classes=3)) == base
    assert sorted(surface_scores(p, t, sp, distances=True)) == sorted(base + ['dist_pred', 'dist_target'])
    assert sorted(surface_scores(p, t, sp, percentiles=(95,))) == sorted(
        base + ['HD', 'HD_pred', 'HD_target', 'HD_pooled', 'percentiles'])
    assert sorted(surface_scores(p, t, sp, tolerances=(1.0,))) == sorted(
        base + ['NSD', 'n_pred_within', 'n_target_within', 'tolerances'])
    assert sorted(case_scores(p, t)) == ['Dice', 'FN', 'FP', 'IoU', 'TN', 'TP']
    assert sorted(case_scores(p, t, spacing=sp)) == ['ASSD', 'Dice', 'FN', 'FP', 'IoU', 'MSSD', 'RAVD', 'TN', 'TP']
    full = case_scores(p, t, spacing=sp, percentiles=(95,), tolerances=(2.0,))
    assert sorted(full) == ['ASSD', 'Dice', 'FN', 'FP', 'HD', 'HD_pooled', 'IoU', 'MSSD', 'NSD', 'RAVD', 'TN', 'TP']
    s = surface_scores(p, t, sp, percentiles=(95,), tolerances=(2.0,))
    assert ss.same_float(full['HD'][0], s['HD'][0]) and ss.same_float(full['NSD'][0], s['NSD'][0])
    # the scores that were there do not move when more is asked for
    plain = surface_scores(p, t, sp)
    for k in base:
        assert ss.same_float(s[k], plain[k]) if k in ('RAVD', 'ASSD', 'MSSD') else s[k] == plain[k]


def test_argument_errors():
    from aide_amd.inference import case_scores
    from aide_amd.utils.metrics3d import surface_scores
    v = np.zeros((3, 4, 5), np.int64)
    for bad in ((), (1, 2, 3, 4, 5), (-1,), (100.5,), (float('nan'),), (float('inf'),), 95, ('x',)):
        with pytest.raises(ValueError):
            surface_scores(v, v, (1, 1, 1), percentiles=bad)
    for bad in ((), (1, 2, 3, 4, 5), (-1e-9,), (float('nan'),), (float('inf'),), 2.0, (None,)):
        with pytest.raises(ValueError):
            surface_scores(v, v, (1, 1, 1), tolerances=bad)
    with pytest.raises(TypeError):
        case_scores(v, v, percentiles=(95,))
    with pytest.raises(TypeError):
        case_scores(v, v, num_classes=3, tolerances=(1.0,))
    with pytest.raises(ValueError):
        case_scores(v, v, spacing=(1, 1, 1), percentiles=(101,))
