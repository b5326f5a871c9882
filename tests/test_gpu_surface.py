"""-m gpu: the surface distances on the device (aide_amd/csrc/surface3d.hip) against the scipy float64 reference of
surface_cases.py, within the bounds derived there: counts, the set of distance entries and RAVD bit-exact; with spacing
(1, 1, 1) every distance and MSSD bit-equal; otherwise 2^-49 relative per distance, and 2^-49 + (n_P + n_T) * 2^-53 for the
sums and ASSD against math.fsum.  Two calls give the same bytes, also on a workspace filled with 0xFF."""
import numpy as np
import pytest
import torch

import surface_cases as sc

pytestmark = pytest.mark.gpu

OTHER_SPACINGS = ((0.7, 0.7, 5.5), (1.37, 1.37, 7.7), (5.5, 0.7, 0.7))
ALL_SPACINGS = ((1.0, 1.0, 1.0),) + OTHER_SPACINGS


def _raw_call(p, t, sp, cls=-1, fill=None):
    """aide_surface3d_scores on two HIP tensors -> (out words int64 [8] on the host, dist [2, ...] on the host)"""
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    out = torch.full((8,), -7, device=p.device, dtype=torch.int64)
    dist = torch.full((2,) + tuple(p.shape), 123.0, device=p.device, dtype=torch.float64)
    ws = torch.empty(lib.aide_surface3d_ws_bytes(p.numel()), device=p.device, dtype=torch.uint8)
    if fill is not None:
        ws.fill_(fill)
    check(lib.aide_surface3d_scores(ptr(p), int(p.dtype == torch.uint8), *p.stride(), ptr(t), int(t.dtype == torch.uint8),
                                    *t.stride(), *p.shape, *sp, cls, ptr(out), ptr(dist), ptr(ws), stream_ptr()), 'surface3d')
    return out.cpu().numpy(), dist.cpu().numpy()


def _as_raw(words, dist):
    f = words[4:].copy().view(np.float64)
    return dict(n_P=words[0], n_T=words[1], V_P=words[2], V_T=words[3], S_PT=f[0], S_TP=f[1], M_PT=f[2], M_TP=f[3],
                dist_P=dist[0], dist_T=dist[1])


def _check(p, t, dev, spacings=ALL_SPACINGS, cls=None, what=''):
    """p, t: numpy volumes, or HIP tensors (any strides) whose logical content is compared"""
    pd, td = (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (p, t))
    pn, tn = pd.cpu().numpy(), td.cpu().numpy()
    for sp in spacings:
        ref = sc.reference(pn, tn, sp, cls)
        words, dist = _raw_call(pd, td, sp, -1 if cls is None else cls)
        sc.check_raw(_as_raw(words, dist), ref, sp, (what, pn.shape, sp))
    return ref


@pytest.mark.parametrize('density', [0.02, 0.3, 0.9])
def test_random_small_shapes(dev, density):
    for k, shape in enumerate(((1, 1, 1), (1, 7, 1), (5, 37, 19), (33, 1, 40), (17, 31, 16))):
        p, t = sc.random_pair(shape, density, seed=1000 * k + int(100 * density))
        _check(p, t, dev, what=density)


@pytest.mark.parametrize('shape', [(520, 2, 3), (2, 520, 3), (3, 2, 520)])
def test_lines_longer_than_a_chunk(dev, shape):
    """a line of 520 in each axis: 17 chunks of 32 candidates and of 32 results, the last one ragged"""
    for density in (0.02, 0.3, 0.9):
        p, t = sc.random_pair(shape, density, seed=int(100 * density) + shape[0])
        _check(p, t, dev, spacings=((1.0, 1.0, 1.0), (5.5, 0.7, 0.7), (0.7, 0.7, 5.5)), what=density)
    # one border voxel at each end of the long axis: the largest distance the volume allows, found across every chunk
    p, t = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    p[0, 0, 0] = 1
    t[-1, -1, -1] = 1
    ref = _check(p, t, dev, what='ends')
    assert ref['n_P'] == ref['n_T'] == 1


@pytest.mark.parametrize('shape', sc.EDGE_SHAPES, ids=['%dx%dx%d' % s for s in sc.EDGE_SHAPES])
def test_chunk_and_workgroup_edges(dev, shape):
    """line lengths around the chunk of 32 and column counts around the workgroup of 64 (surface_cases.EDGE_SHAPES), int64 and
    uint8, a permuted view, a volume that is all border and one without any"""
    for density in (0.3, 0.9):
        p, t = sc.random_pair(shape, density, seed=shape[0] + 7 * shape[1] + int(10 * density))
        _check(p, t, dev, what=('edges', density))
        _check(p.astype(np.uint8), t, dev, spacings=((5.5, 0.7, 0.7),), what=('edges uint8', density))
        view = torch.from_numpy(np.ascontiguousarray(p.transpose(2, 0, 1))).to(dev).permute(1, 2, 0)     # [S,H,W] storage
        assert tuple(view.shape) == shape
        _check(view, torch.from_numpy(t).to(dev), dev, spacings=((0.7, 0.7, 5.5),), what=('edges permuted', density))
    full, zero = np.ones(shape, np.int64), np.zeros(shape, np.int64)
    part, _ = sc.random_pair(shape, 0.5, seed=shape[2])
    ref = _check(full, full, dev, what='edges full / full')
    assert min(shape) > 2 or ref['n_P'] == full.size      # a dim of 1 or 2: every voxel is a border voxel, every f is 0
    _check(full, part, dev, what='edges full / random')
    for a, b in ((zero, part), (part, zero)):             # one side without a border voxel: every f is +inf
        words, dist = _raw_call(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), (0.7, 0.7, 5.5))
        sc.check_raw(_as_raw(words, dist), sc.reference(a, b, (0.7, 0.7, 5.5)), (0.7, 0.7, 5.5), 'edges empty')
        assert np.all(dist == -1.0) and np.all(words[4:] == 0)


def test_ellipsoid_pairs(dev):
    for shape, spacings in (((64, 64, 33), ALL_SPACINGS), ((256, 256, 33), ((1.37, 1.37, 7.7),))):
        p, t = sc.ellipsoid_pair(shape)
        ref = _check(p, t, dev, spacings=spacings, what='ellipsoid')
        assert ref['n_P'] > 0 and ref['n_T'] > 0 and ref['V_P'] > ref['n_P']


def test_corner_blobs_full_and_empty(dev):
    p, t = sc.corner_blobs(40)
    _check(p, t, dev, what='corners')
    full = np.ones((9, 20, 11), np.int64)
    part, _ = sc.random_pair(full.shape, 0.3, seed=5)
    _check(full, full, dev, what='full / full')
    _check(full, part, dev, what='full / random')
    zero = np.zeros_like(full)
    for a, b in ((zero, part), (part, zero), (zero, zero)):
        for sp in ((1.0, 1.0, 1.0), (0.7, 0.7, 5.5)):
            words, dist = _raw_call(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), sp)
            ref = sc.reference(a, b, sp)
            sc.check_raw(_as_raw(words, dist), ref, sp, 'empty')
            assert np.all(dist == -1.0) and np.all(words[4:] == 0)


def test_layouts_and_dtypes(dev):
    sp = (0.7, 0.7, 5.5)
    p, t = sc.random_pair((12, 21, 10), 0.3, seed=21)
    for dp in (np.uint8, np.int64):
        for dt in (np.uint8, np.int64):
            _check(p.astype(dp), t.astype(dt), dev, spacings=(sp,), what=(dp, dt))
    # [S,H,W] labels passed as the reference's [H,W,S] view, against a contiguous [H,W,S] target
    shw = torch.from_numpy(np.ascontiguousarray(p.transpose(2, 0, 1))).to(dev)
    view = shw.permute(1, 2, 0)
    assert not view.is_contiguous()
    _check(view, torch.from_numpy(t).to(dev), dev, what='permuted')
    # every second plane of a larger tensor (uint8 and int64), against a permuted target
    big_p, big_t = sc.random_pair((24, 21, 10), 0.3, seed=22, dtype=np.uint8)
    tt = torch.from_numpy(np.ascontiguousarray(big_t[::2].astype(np.int64).transpose(1, 0, 2))).to(dev).permute(1, 0, 2)
    _check(torch.from_numpy(big_p).to(dev)[::2], tt, dev, what='slice view')


def test_classes_on_device(dev):
    from aide_amd.utils.metrics3d import surface_scores
    sp = (1.37, 1.37, 7.7)
    for dtype in (np.int64, np.uint8):
        p, t = sc.class_pair((9, 37, 12), seed=31, dtype=dtype)
        for c in range(1, 5):
            _check(p, t, dev, spacings=(sp, (1.0, 1.0, 1.0)), cls=c, what=(dtype, c))
        s = surface_scores(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev), sp, num_classes=5, distances=True)
        assert s['dist_pred'].is_cuda and tuple(s['dist_pred'].shape) == (5, 9, 37, 12)
        assert bool((s['dist_pred'][0] == -1.0).all()) and bool((s['dist_pred'][3] == -1.0).all())
        for k in ('RAVD', 'ASSD', 'MSSD'):
            assert s[k].shape == (5,) and np.isnan(s[k][0]) and np.isnan(s[k][3])            # background, absent class
        for c in (1, 2, 4):
            ref = sc.reference(p, t, sp, c)
            sc.check_scores({k: v[c] for k, v in s.items() if not k.startswith('dist')}, ref, sp, (dtype, c))
            sc.check_raw(dict(ref, dist_P=s['dist_pred'][c].cpu().numpy(), dist_T=s['dist_target'][c].cpu().numpy()), ref, sp, c)


def test_deterministic_whatever_the_workspace_held(dev):
    p, t = sc.ellipsoid_pair((40, 70, 33))
    pd, td = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
    for sp in ((1.0, 1.0, 1.0), (1.37, 1.37, 7.7)):
        w0, d0 = _raw_call(pd, td, sp, fill=0)
        w1, d1 = _raw_call(pd, td, sp)
        w2, d2 = _raw_call(pd, td, sp, fill=0xFF)
        assert w0.tobytes() == w1.tobytes() == w2.tobytes()
        assert d0.tobytes() == d1.tobytes() == d2.tobytes()
        assert w0[0] > 0 and w0[1] > 0


def test_python_layer_on_device(dev):
    from aide_amd.utils.metrics3d import surface_scores, ASSD3d_fn, MSSD3d_fn, RAVD3d_fn
    sp = (0.7, 0.7, 5.5)
    p, t = sc.ellipsoid_pair((20, 24, 9))
    pd, td = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
    ref = sc.reference(p, t, sp)
    s = surface_scores(pd, td, sp, distances=True)
    sc.check_scores(s, ref, sp)
    assert s['dist_pred'].is_cuda and s['dist_pred'].dtype == torch.float64 and tuple(s['dist_pred'].shape) == p.shape
    sc.check_raw(dict(ref, dist_P=s['dist_pred'].cpu().numpy(), dist_T=s['dist_target'].cpu().numpy()), ref, sp)
    assert sorted(surface_scores(pd, td, sp)) == ['ASSD', 'MSSD', 'RAVD', 'V_pred', 'V_target', 'n_pred', 'n_target']
    assert sc.same_float(ASSD3d_fn(pd, td, sp), s['ASSD']) and sc.same_float(MSSD3d_fn(pd, td, sp), s['MSSD'])
    assert sc.same_float(RAVD3d_fn(pd, t), s['RAVD'])                        # a numpy operand follows the HIP one
    empty = torch.zeros(0, 4, 4, dtype=torch.int64, device=dev)
    e = surface_scores(empty, empty, sp)
    assert np.isnan(e['ASSD']) and np.isnan(e['RAVD']) and e['n_pred'] == 0
    with pytest.raises(ValueError):
        surface_scores(pd, td, (1.0, 0.0, 1.0))
    with pytest.raises(RuntimeError):
        surface_scores(pd, td[:, :, :5], sp)
    with pytest.raises(RuntimeError):
        surface_scores(pd.double(), td, sp)


def test_predicted_case_end_to_end(dev):
    """predict_case(keep_largest=True, numpy=False) on a synthetic 8-slice case, then case_scores with a spacing: the host
    path on the copied volumes within the same bounds; without `spacing` the keys are what they were."""
    from aide_amd.inference import case_scores, predict_case
    from aide_amd.models_twomodalinputs import fuseunet
    from aide_amd.synthetic import chaos_batch
    torch.manual_seed(3)
    net = fuseunet(2).to(dev).eval()
    xin, xout, tgt = chaos_batch(8, 64, seed=77)
    keep = predict_case(net, xin.to(dev), xout.to(dev), keep_largest=True, numpy=False)
    target = tgt.to(dev).permute(1, 2, 0)
    sp = (1.4, 1.4, 7.0)
    got = case_scores(keep, target, spacing=sp)
    assert sorted(got) == ['ASSD', 'Dice', 'FN', 'FP', 'IoU', 'MSSD', 'RAVD', 'TN', 'TP']
    kn, tn = keep.cpu().numpy(), target.cpu().numpy()
    host = case_scores(kn, tn, spacing=sp)
    ref = sc.reference(kn, tn, sp)
    counts = dict(n_pred=ref['n_P'], n_target=ref['n_T'], V_pred=ref['V_P'], V_target=ref['V_T'])
    sc.check_scores(dict(got, **counts), ref, sp, 'device')
    sc.check_scores(dict(host, **counts), ref, sp, 'host')
    for k in ('Dice', 'IoU'):
        assert sc.same_float(got[k], host[k])
    for k in ('TP', 'TN', 'FP', 'FN'):
        assert got[k] == host[k]
    assert sorted(case_scores(keep, target)) == ['Dice', 'FN', 'FP', 'IoU', 'TN', 'TP']
