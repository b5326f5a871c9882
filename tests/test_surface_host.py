"""Host side of the spacing-aware case metrics (aide_amd/utils/metrics3d.py, include/aide_hip.h "surface distances"): the
scipy path equals an O(n^2) numpy evaluation of the definitions, hand cases, the empty rules, RAVD bit for bit, class arrays,
argument errors, and case_scores without `spacing` is what it was.  No device."""
import math

import numpy as np
import pytest
import torch

import surface_cases as sc


@pytest.fixture(scope='module')
def built():
    from aide_amd.build import build
    return build(verbose=False)


def _host_raw(p, t, sp):
    """the host path's raw values under the keys of surface_cases (S from the maps with fsum, as the reference does)"""
    from aide_amd.utils.metrics3d import surface_scores
    s = surface_scores(p, t, sp, distances=True)
    dp, dt = s['dist_pred'], s['dist_target']
    assert isinstance(dp, np.ndarray) and dp.dtype == np.float64 and dp.shape == np.shape(p)
    vp, vt = dp[dp >= 0], dt[dt >= 0]
    raw = dict(n_P=s['n_pred'], n_T=s['n_target'], V_P=s['V_pred'], V_T=s['V_target'],
               S_PT=math.fsum(vp.tolist()), S_TP=math.fsum(vt.tolist()), M_PT=vp.max() if vp.size else 0.0,
               M_TP=vt.max() if vt.size else 0.0, dist_P=dp, dist_T=dt)
    return raw, s


@pytest.mark.parametrize('spacing', sc.SPACINGS)
def test_reference_and_host_path_equal_brute(spacing):
    for k, shape in enumerate(sc.SMALL_SHAPES):
        # (0.9 on the largest shape would be 4000 x 4000 border pairs per direction: the smaller shapes cover dense volumes)
        for density in (0.05, 0.3, 0.9)[:2 if shape == (17, 31, 16) else 3]:
            p, t = sc.random_pair(shape, density, seed=100 * k + int(10 * density))
            ref = sc.brute(p, t, spacing)
            what = (shape, density, spacing)
            sc.check_raw(sc.reference(p, t, spacing), ref, spacing, what)
            raw, scores = _host_raw(p, t, spacing)
            sc.check_raw(raw, ref, spacing, what)
            sc.check_scores(scores, ref, spacing, what)


def test_hand_cases():
    from aide_amd.utils.metrics3d import surface_scores, ASSD3d_fn, MSSD3d_fn, RAVD3d_fn
    p, t = np.zeros((6, 7, 5), np.int64), np.zeros((6, 7, 5), np.int64)
    p[1, 2, 3] = 1
    t[3, 5, 4] = 1
    s = surface_scores(p, t, (0.5, 2, 3))
    assert s['ASSD'] == math.sqrt(46.0) and s['MSSD'] == math.sqrt(46.0) and s['RAVD'] == 0.0
    assert (s['n_pred'], s['n_target'], s['V_pred'], s['V_target']) == (1, 1, 1, 1)
    assert ASSD3d_fn(p, t, (0.5, 2, 3)) == math.sqrt(46.0) and MSSD3d_fn(p, t) == math.sqrt(4 + 9 + 1)
    p, _ = sc.ellipsoid_pair((12, 14, 9))
    s = surface_scores(p, p.copy(), (0.7, 0.7, 5.5))
    assert s['ASSD'] == 0.0 and s['MSSD'] == 0.0 and s['RAVD'] == 0.0 and s['n_pred'] == s['n_target'] > 0
    cube = np.ones((5, 5, 5), np.uint8)
    assert surface_scores(cube, cube, (1, 1, 1))['n_pred'] == 98
    slab = np.ones((1, 4, 4), np.uint8)
    assert surface_scores(slab, slab, (1, 1, 1))['n_target'] == 16
    half = np.zeros((2, 2, 3), np.int64)
    half[0] = 1
    assert RAVD3d_fn(np.ones((2, 2, 3), np.int64), half) == 100.0           # |12 - 6| / 6 * 100
    # torch CPU tensors take the same path
    s2 = surface_scores(torch.from_numpy(cube), torch.from_numpy(cube), (1, 1, 1))
    assert s2['n_pred'] == 98 and s2['MSSD'] == 0.0


def test_empty_rules():
    from aide_amd.utils.metrics3d import surface_scores
    z, one = np.zeros((3, 4, 5), np.int64), np.zeros((3, 4, 5), np.int64)
    one[1, 1:3, 2] = 1
    s = surface_scores(z, one, (1, 2, 3), distances=True)                  # empty prediction
    assert np.isnan(s['ASSD']) and np.isnan(s['MSSD']) and s['RAVD'] == 100.0 and s['n_pred'] == 0 and s['n_target'] == 2
    assert np.all(s['dist_pred'] == -1.0) and np.all(s['dist_target'] == -1.0)
    s = surface_scores(one, z, (1, 2, 3))                                  # empty target: x / 0 -> inf
    assert np.isnan(s['ASSD']) and np.isnan(s['MSSD']) and np.isinf(s['RAVD']) and s['RAVD'] > 0
    s = surface_scores(z, z, (1, 2, 3))                                    # both empty: 0 / 0 -> nan
    assert np.isnan(s['ASSD']) and np.isnan(s['MSSD']) and np.isnan(s['RAVD'])


def test_ravd_bit_for_bit():
    from aide_amd.utils.metrics3d import surface_scores
    rng = np.random.RandomState(3)
    for _ in range(20):
        p, t = (rng.rand(4, 9, 7) < rng.rand()).astype(np.int64), (rng.rand(4, 9, 7) < rng.rand()).astype(np.int64)
        vp, vt = int(p.sum()), int(t.sum())
        with np.errstate(divide='ignore', invalid='ignore'):
            want = np.float64(abs(vp - vt)) / np.float64(vt) * 100.0
        assert sc.same_float(surface_scores(p, t, (1.37, 1.37, 7.7))['RAVD'], want)


def test_classes_absent_and_out_of_range():
    from aide_amd.utils.metrics3d import surface_scores
    sp = (0.7, 0.7, 5.5)
    for dtype in (np.int64, np.uint8):
        p, t = sc.class_pair((9, 12, 7), seed=4, dtype=dtype)
        s = surface_scores(p, t, sp, num_classes=5, distances=True)
        for k in ('RAVD', 'ASSD', 'MSSD'):
            assert s[k].shape == (5,) and s[k].dtype == np.float64 and np.isnan(s[k][0])
        assert s['dist_pred'].shape == (5, 9, 12, 7) and np.all(s['dist_pred'][0] == -1.0)
        for c in range(1, 5):
            ref = sc.brute(p, t, sp, cls=c)
            sc.check_scores({k: v[c] for k, v in s.items() if not k.startswith('dist')}, ref, sp, (dtype, c))
            sc.check_raw(dict(ref, dist_P=s['dist_pred'][c], dist_T=s['dist_target'][c]), ref, sp, (dtype, c))
        assert s['n_pred'][3] == 0 and s['V_target'][3] == 0 and np.isnan(s['ASSD'][3]) and np.isnan(s['RAVD'][3])   # absent
        assert s['V_pred'][1:].sum() < np.count_nonzero(p)                  # the out-of-range labels belong to no class


def test_argument_errors():
    from aide_amd.utils.metrics3d import surface_scores
    v = np.zeros((3, 4, 5), np.int64)
    for bad in ((1, 1), (1, 1, 1, 1), (0, 1, 1), (1, -2, 1), (1, 1, float('nan')), (1, float('inf'), 1), 3.0, None):
        with pytest.raises(ValueError):
            surface_scores(v, v, bad)
    with pytest.raises(RuntimeError):
        surface_scores(v, np.zeros((3, 4, 6), np.int64), (1, 1, 1))
    with pytest.raises(RuntimeError):
        surface_scores(v[0], v[0], (1, 1, 1))
    with pytest.raises(RuntimeError):
        surface_scores(v, v, (1, 1, 1), num_classes=9)


def test_entry_point_rejects_without_launch(built):
    """Answered on the host, before any HIP call (no device here)."""
    import ctypes
    from aide_amd._lib import lib, parse_header
    protos = parse_header()
    assert len(protos['aide_surface3d_scores'][1]) == 21 and len(protos['aide_surface3d_ws_bytes'][1]) == 1
    assert lib.aide_surface3d_ws_bytes(2 ** 31) == 0 and lib.aide_surface3d_ws_bytes(-1) == 0
    assert lib.aide_surface3d_ws_bytes(1000) >= 1000 * (2 * 8 + 2 * 4 + 2) + 64
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    assert a % 16 == 0 or (a + 8) % 16 == 0
    a += a % 16                                                             # 16-byte aligned inside buf
    ok = dict(p=a, t=a, dims=(2, 2, 2), sp=(1.0, 1.0, 1.0), out=a, ws=a)

    def call(**kw):
        q = dict(ok, **kw)
        return lib.aide_surface3d_scores(q['p'], 0, 4, 2, 1, q['t'], 0, 4, 2, 1, *q['dims'], *q['sp'], -1, q['out'], None, q['ws'],
                                         None)
    for kw in (dict(p=None), dict(t=None), dict(out=None), dict(ws=None), dict(ws=a + 8), dict(dims=(2 ** 16, 2 ** 15, 1)),
               dict(dims=(-1, 2, 2)), dict(sp=(0.0, 1.0, 1.0)), dict(sp=(1.0, -1.0, 1.0)), dict(sp=(1.0, 1.0, float('nan'))),
               dict(sp=(float('inf'), 1.0, 1.0))):
        assert call(**kw) < 0, kw


def test_case_scores_without_spacing_is_unchanged():
    from aide_amd.inference import case_scores
    p, t = sc.random_pair((6, 9, 5), 0.4, seed=8)
    s = case_scores(p, t)
    assert sorted(s) == ['Dice', 'FN', 'FP', 'IoU', 'TN', 'TP']
    assert sorted(case_scores(p, t, num_classes=3)) == ['Dice', 'FN', 'FP', 'IoU', 'TN', 'TP']
    sp = (1.4, 1.4, 7.0)
    s2 = case_scores(p, t, spacing=sp)
    assert sorted(s2) == ['ASSD', 'Dice', 'FN', 'FP', 'IoU', 'MSSD', 'RAVD', 'TN', 'TP']
    for k in s:
        assert sc.same_float(s2[k], s[k]) if k in ('Dice', 'IoU') else s2[k] == s[k]
    ref = sc.brute(p, t, sp)
    sc.check_scores(dict(s2, n_pred=ref['n_P'], n_target=ref['n_T'], V_pred=ref['V_P'], V_target=ref['V_T']), ref, sp)
    s3 = case_scores(p, t, num_classes=3, spacing=sp)
    assert s3['ASSD'].shape == (3,) and np.isnan(s3['ASSD'][0]) and s3['Dice'].shape == (3,)


def test_reference_module_functions():
    """utils/metrics3d.py carries the evaluation script's three functions (evalchaos_comparison_1cases.py:116-141)."""
    from aide_amd.utils import surface_scores                               # noqa: F401  (exported)
    from aide_amd.utils.metrics3d import Dice3d_fn, IoU3d_fn, TP_TN_FP_FN3d
    p, t = sc.random_pair((6, 9, 5), 0.4, seed=9)
    i, f = p.reshape(-1), t.reshape(-1)
    assert Dice3d_fn(p, t) == 2 * np.sum(i * f) / (np.sum(i) + np.sum(f))
    assert IoU3d_fn(p, t) == np.sum(i * f) / (np.sum(i) + np.sum(f) - np.sum(i * f))
    assert TP_TN_FP_FN3d(p, t) == (np.sum(i * f), np.sum((1 - i) * (1 - f)), np.sum(i * (1 - f)), np.sum((1 - i) * f))
