"""-m gpu: percentiles of the surface distances (HD95) and tolerance counts (NSD) on the device
(aide_surface3d_scores_select, aide_amd/csrc/surface3d.hip) against np.sort of the scipy float64 reference distances, within
the bounds surface_select_cases.py derives: counts exact, percentiles bit-equal at spacing (1, 1, 1) and 2^-49 relative
otherwise.  The eight old words and the distance map are the old entry's bytes; two calls give the same 52 words whatever the
workspace held."""
import ctypes

import numpy as np
import pytest
import torch

import surface_select_cases as ss

pytestmark = pytest.mark.gpu

WORDS = 52


def _raw_select(p, t, sp, qs=(), taus=(), cls=-1, fill=None, with_dist=True):
    """aide_surface3d_scores_select on two HIP tensors -> (out words int64 [52] on the host, dist [2, ...] or None);
    fill: None, a byte value, or 'random' for the workspace's content before the call"""
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    out = torch.full((WORDS,), -7, device=p.device, dtype=torch.int64)
    dist = torch.full((2,) + tuple(p.shape), 123.0, device=p.device, dtype=torch.float64) if with_dist else None
    ws = torch.empty(lib.aide_surface3d_select_ws_bytes(p.numel()), device=p.device, dtype=torch.uint8)
    if fill == 'random':
        ws.copy_(torch.randint(0, 256, (ws.numel(),), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)))
    elif fill is not None:
        ws.fill_(fill)
    cq, ct = (ctypes.c_double * 4)(*qs), (ctypes.c_double * 4)(*taus)
    check(lib.aide_surface3d_scores_select(ptr(p), int(p.dtype == torch.uint8), *p.stride(), ptr(t), int(t.dtype == torch.uint8),
                                           *t.stride(), *p.shape, *sp, cls, cq, len(qs), ct, len(taus), ptr(out),
                                           ptr(dist) if with_dist else None, ptr(ws), stream_ptr()), 'surface3d_select')
    return out.cpu().numpy(), dist.cpu().numpy() if with_dist else None


def _raw_old(p, t, sp, cls=-1, with_dist=True):
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    out = torch.full((8,), -7, device=p.device, dtype=torch.int64)
    dist = torch.full((2,) + tuple(p.shape), 123.0, device=p.device, dtype=torch.float64) if with_dist else None
    ws = torch.empty(lib.aide_surface3d_ws_bytes(p.numel()), device=p.device, dtype=torch.uint8)
    check(lib.aide_surface3d_scores(ptr(p), int(p.dtype == torch.uint8), *p.stride(), ptr(t), int(t.dtype == torch.uint8),
                                    *t.stride(), *p.shape, *sp, cls, ptr(out), ptr(dist) if with_dist else None, ptr(ws),
                                    stream_ptr()), 'surface3d')
    return out.cpu().numpy(), dist.cpu().numpy() if with_dist else None


def _dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _check_case(p, t, sp, dev, what=''):
    """both percentile sets and the case's tolerances through surface_scores on HIP tensors, against the reference"""
    from aide_amd.utils.metrics3d import surface_scores
    ref = ss.reference(p, t, sp)
    taus = ss.taus_for(ref, sp)
    pd, td = _dev(p, dev), _dev(t, dev)
    for qs in ss.QS:
        got = surface_scores(pd, td, sp, percentiles=qs, tolerances=taus)
        ss.check_select(got, ref, sp, qs, taus, (what, sp, qs))
    return ref, pd, td


@pytest.mark.parametrize('spacing', ss.SPACINGS)
def test_small_shapes(dev, spacing):
    for shape, p, t in ss.small_cases():
        ref, pd, td = _check_case(p, t, spacing, dev, shape)
        assert ref['n_P'] >= 3 and ref['n_T'] >= 3
        # q = 100 is the maximum of the same call, bit for bit, in both directions
        words, _ = _raw_select(pd, td, spacing, qs=(100.0,))
        tri = words[16:].reshape(3, 4, 3)
        assert tri[0, 0, 0] == ref['n_P'] - 1 and tri[1, 0, 0] == ref['n_T'] - 1 and tri[2, 0, 0] == ref['n_P'] + ref['n_T'] - 1
        assert tri[0, 0, 1] == tri[0, 0, 2] == words[6] and tri[1, 0, 1] == tri[1, 0, 2] == words[7]      # M_PT, M_TP
        assert tri[2, 0, 1] == max(words[6], words[7])                       # (non-negative doubles order like their bits)


@pytest.mark.parametrize('spacing', [ss.UNIT, (0.7, 0.7, 5.5)])
def test_old_words_and_dist_are_the_old_bytes(dev, spacing):
    _, p, t = list(ss.small_cases())[3]
    pd, td = _dev(p, dev), _dev(t.astype(np.uint8), dev)
    for with_dist in (True, False):
        w_old, d_old = _raw_old(pd, td, spacing, with_dist=with_dist)
        for qs, taus in (((), ()), ((95.0,), (1.0, 2.0)), ((0.0, 25.0, 50.0, 95.0), (0.0, 1.0, 2.0, 3.0))):
            w, d = _raw_select(pd, td, spacing, qs, taus, with_dist=with_dist)
            assert w[:8].tobytes() == w_old.tobytes(), (with_dist, qs)
            if with_dist:
                assert d.tobytes() == d_old.tobytes()
            if not qs:
                assert not w[8:].any()                                      # nothing asked for: the old entry's result


@pytest.mark.parametrize('spacing', [ss.UNIT, (0.7, 0.7, 5.5)])
def test_lists_over_many_workgroups(dev, spacing):
    """more than 65 536 keys per list: every workgroup of the histogram launch has work, slots beyond 2^16; at unit spacing
    a few values hold almost all keys"""
    p, t = ss.random_pair((40, 64, 64), 0.5, seed=11)
    ref, pd, td = _check_case(p, t, spacing, dev, 'large')
    assert ref['n_P'] > 65536 and ref['n_T'] > 65536


def test_degenerate_cases(dev):
    from aide_amd.utils.metrics3d import surface_scores, HD95_fn, NSD3d_fn
    qs, taus = (0.0, 50.0, 95.0, 100.0), (0.0, 1.0)
    # one border voxel each: m = 1, pooled m = 2
    p, t = np.zeros((6, 7, 5), np.int64), np.zeros((6, 7, 5), np.int64)
    p[1, 2, 3] = 1
    t[3, 5, 4] = 1
    for sp in (ss.UNIT, (0.5, 2.0, 3.0)):             # sqrt(46) also with the spacing: every product, square and sum is an
        ref = ss.reference(p, t, sp)                  # integer, so the one distance is attained exactly as a tolerance
        got = surface_scores(_dev(p, dev), _dev(t, dev), sp, percentiles=qs, tolerances=(float(ref['M_PT']), 1.0))
        ss.check_select(got, ref, sp, qs, (float(ref['M_PT']), 1.0), 'single voxels')
    # empty prediction, empty target, both
    one, zero = np.zeros((9, 20, 11), np.int64), np.zeros((9, 20, 11), np.int64)
    one[2:5, 3:9, 4] = 1
    for a, b in ((zero, one), (one, zero), (zero, zero)):
        words, _ = _raw_select(_dev(a, dev), _dev(b, dev), (0.7, 0.7, 5.5), qs, taus)
        assert not words[4:].any()
        got = surface_scores(_dev(a, dev), _dev(b, dev), (0.7, 0.7, 5.5), percentiles=qs, tolerances=taus)
        for k in ('HD', 'HD_pred', 'HD_target', 'HD_pooled'):
            assert got[k].shape == (4,) and np.all(np.isnan(got[k]))
        assert np.all(np.isnan(got['NSD'])) and not got['n_pred_within'].any() and not got['n_target_within'].any()
    # identical volumes
    e, _ = ss.ellipsoid_pair((20, 24, 9))
    got = surface_scores(_dev(e, dev), _dev(e, dev), (1.37, 1.37, 7.7), percentiles=qs, tolerances=(0.0,))
    for k in ('HD', 'HD_pred', 'HD_target', 'HD_pooled'):
        assert np.all(got[k] == 0.0) and not np.signbit(got[k]).any()
    assert got['NSD'][0] == 1.0 and got['n_pred_within'][0] == got['n_pred']
    # corner blobs, a single line, an empty volume
    p, t = ss.corner_blobs(40)
    for sp in (ss.UNIT, (1.37, 1.37, 7.7)):
        _check_case(p, t, sp, dev, 'corners')
    _, p, t = list(ss.small_cases())[1]
    assert p.shape == (1, 7, 1)
    _check_case(p, t, (1.37, 1.37, 7.7), dev, 'line')
    none = torch.zeros(0, 4, 4, dtype=torch.int64, device=dev)
    got = surface_scores(none, none, ss.UNIT, percentiles=(95,), tolerances=(1.0,))
    assert np.isnan(got['HD'][0]) and np.isnan(got['NSD'][0])
    assert ss.same_float(HD95_fn(_dev(e, dev), _dev(e, dev)), 0.0) and NSD3d_fn(_dev(e, dev), _dev(e, dev), 0.0) == 1.0


def test_strided_and_typed_operands(dev):
    sp = (0.7, 0.7, 5.5)
    p, t = ss.random_pair((12, 21, 10), 0.3, seed=21, dtype=np.uint8)
    qs, taus = (25.0, 95.0), ss.taus_for(ss.reference(p, t, sp), sp)
    shw = _dev(p.transpose(2, 0, 1), dev)
    view = shw.permute(1, 2, 0)
    assert not view.is_contiguous() and view.dtype == torch.uint8
    w_view, d_view = _raw_select(view, _dev(t, dev), sp, qs, taus)
    w_cont, d_cont = _raw_select(_dev(p.astype(np.int64), dev), _dev(t.astype(np.int64), dev), sp, qs, taus)
    assert w_view.tobytes() == w_cont.tobytes() and d_view.tobytes() == d_cont.tobytes()
    assert w_view[0] > 0 and w_view[16 + 3 + 1] > 0                        # x[lo] of the 95th percentile of A


def test_classes_and_case_scores(dev):
    from aide_amd.inference import case_scores
    from aide_amd.utils.metrics3d import surface_scores
    sp = (1.37, 1.37, 7.7)
    p, t = ss.class_pair((17, 31, 16), seed=31)
    qs = (50.0, 95.0)
    refs = {c: ss.reference(p, t, sp, c) for c in (1, 2, 3, 4)}
    assert refs[3]['n_P'] == 0 and refs[3]['n_T'] == 0
    taus = ss.taus_for(refs[1], sp, count=1)
    for c in (2, 4):                                                        # the condition on tau, for every class it is used on
        ab = ss.lists(refs[c])[2]
        assert np.all(np.abs(ab - taus[0]) > 2.0 * ss.REL * taus[0])
    pd, td = _dev(p, dev), _dev(t, dev)
    s = surface_scores(pd, td, sp, num_classes=5, percentiles=qs, tolerances=taus)
    for k in ('HD', 'HD_pred', 'HD_target', 'HD_pooled'):
        assert s[k].shape == (5, 2) and np.all(np.isnan(s[k][0])) and np.all(np.isnan(s[k][3]))
    assert s['NSD'].shape == (5, 1) and np.isnan(s['NSD'][0, 0]) and np.isnan(s['NSD'][3, 0])
    assert s['n_pred_within'].dtype == np.int64 and s['n_pred_within'][0, 0] == 0 and s['n_target_within'][3, 0] == 0
    for c in (1, 2, 4):
        row = {k: (v if k in ('percentiles', 'tolerances') else v[c]) for k, v in s.items()}
        ss.check_select(row, refs[c], sp, qs, taus, c)
    cs = case_scores(pd, td, num_classes=5, spacing=sp, percentiles=(95.0,), tolerances=taus)
    assert sorted(cs) == ['ASSD', 'Dice', 'FN', 'FP', 'HD', 'HD_pooled', 'IoU', 'MSSD', 'NSD', 'RAVD', 'TN', 'TP']
    assert cs['HD'].shape == (5, 1) and cs['NSD'].shape == (5, 1)
    for c in (1, 2, 4):
        assert ss.same_float(cs['HD'][c, 0], s['HD'][c, 1]) and ss.same_float(cs['HD_pooled'][c, 0], s['HD_pooled'][c, 1])
        assert ss.same_float(cs['NSD'][c, 0], s['NSD'][c, 0])
    with pytest.raises(TypeError):
        case_scores(pd, td, percentiles=(95.0,))
    with pytest.raises(ValueError):
        surface_scores(pd, td, sp, percentiles=(101.0,))


def test_same_words_whatever_the_workspace_held(dev):
    p, t = ss.ellipsoid_pair((40, 70, 33))
    pd, td = _dev(p, dev), _dev(t, dev)
    qs, taus = (0.0, 50.0, 95.0, 100.0), (1.0, 2.0, 3.5)
    for sp in (ss.UNIT, (1.37, 1.37, 7.7)):
        w0, d0 = _raw_select(pd, td, sp, qs, taus, fill=0)
        w1, d1 = _raw_select(pd, td, sp, qs, taus, fill=0xFF)
        w2, d2 = _raw_select(pd, td, sp, qs, taus, fill='random')
        w3, d3 = _raw_select(pd, td, sp, qs, taus, fill='random')
        assert w0.tobytes() == w1.tobytes() == w2.tobytes() == w3.tobytes()
        assert d0.tobytes() == d1.tobytes() == d2.tobytes() == d3.tobytes()
        assert w0[0] > 0 and w0[1] > 0 and w0[8] > 0 and w0[17] >= 0
