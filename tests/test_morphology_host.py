"""CPU: the numpy path of aide_amd/morphology.py (scipy, the definition) equals the brute force of morphology_cases for all five
operations, binary and per class; ball() is the expression; opening is anti-extensive and closing extensive for every case and
radius; the distance transform and its +inf convention; argument validation."""
import numpy as np
import pytest
import torch

import morphology_cases as mc

CASES, CLASS_CASES = mc.cases(), mc.class_cases()


def _call(m, vol, op, r, sp, classes=None):
    if op == 'erode0':
        return m.erode(vol, r, sp, classes, outside=0)
    if op == 'erode1':
        return m.erode(vol, r, sp, classes, outside=1)
    return {'dilate': m.dilate, 'open': m.open_, 'close': m.close}[op](vol, r, sp, classes)


@pytest.mark.parametrize('index', range(len(CASES)), ids=[c.name for c in CASES])
def test_numpy_path_equals_brute_force(index):
    from aide_amd import morphology as m
    vol = CASES[index].volume
    for setting, (sp, r) in enumerate(mc.SETTINGS):
        for op in mc.OPS:
            got = _call(m, vol, op, r, sp)
            want = mc.reference('binary', index, op, setting)
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == vol.shape
            assert np.array_equal(got, want), (CASES[index].name, op, sp, r, int((got != want).sum()))
        x = (vol != 0)
        opened, closed = mc.reference('binary', index, 'open', setting), mc.reference('binary', index, 'close', setting)
        assert not (opened.astype(bool) & ~x).any(), (CASES[index].name, sp, r)       # open is a subset of X
        assert not (x & ~closed.astype(bool)).any(), (CASES[index].name, sp, r)       # X is a subset of close


@pytest.mark.parametrize('index', range(len(CLASS_CASES)), ids=[c.name for c in CLASS_CASES])
def test_numpy_path_classes_equal_brute_force(index):
    from aide_amd import morphology as m
    case = CLASS_CASES[index]
    for setting, (sp, r) in enumerate(mc.SETTINGS):
        for op in mc.OPS:
            got = _call(m, case.volume, op, r, sp, case.classes)
            want = mc.reference('classes', index, op, setting)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (case.name, op, sp, r, int((got != want).sum()))
            assert got.max() < case.classes
        inrange = (case.volume >= 1) & (case.volume < case.classes)
        for op in ('dilate', 'close'):            # a class is never overwritten
            want = mc.reference('classes', index, op, setting)
            assert np.array_equal(want[inrange], case.volume[inrange]), (case.name, op, sp, r)
        opened = mc.reference('classes', index, 'open', setting)
        assert np.array_equal(opened[opened != 0], case.volume[opened != 0]), (case.name, sp, r)


def test_contested_voxels_and_binary_as_two_classes():
    from aide_amd import morphology as m
    vol = CLASS_CASES[0].volume                   # classes 1 and 2, row 7 between them
    got = m.dilate(vol, 1.0, mc.UNIT, 3)
    assert (got[:, 7, 3:13] == 0).all() and (got[:, 1, 3:13] == 1).all() and (got[:, 14, 3:13] == 2).all()
    assert (m.dilate(vol, 1.0, mc.UNIT)[:, 7, 3:13] == 1).all()
    for case in CASES[:5]:
        for op in mc.OPS:
            assert np.array_equal(_call(m, case.volume, op, 1.5, mc.SPACING, 2), _call(m, case.volume, op, 1.5, mc.SPACING))
    t = torch.from_numpy(CASES[3].volume)         # a CPU tensor takes the numpy path
    assert np.array_equal(m.open_(t, 2.0), m.open_(CASES[3].volume, 2.0))


def test_ball_is_the_expression():
    from aide_amd.morphology import ball
    for sp, r in mc.SETTINGS + ((mc.SPACING, 0.0), ((1.37, 1.37, 7.7), 3.0), ((1.37, 1.37, 7.7), 10.0)):
        b = ball(r, sp)
        assert b.dtype == np.bool_ and all(s % 2 == 1 for s in b.shape)
        w = tuple(s // 2 for s in b.shape)
        assert all(a <= c for a, c in zip(w, mc.reach(r, sp)))
        inside = {tuple(int(i) - k for i, k in zip(idx, w)) for idx in np.argwhere(b)}
        assert inside == set(mc.offsets(r, sp)), (sp, r)
        assert b[w] and b.sum() == len(inside)
    assert ball(0.0).shape == (1, 1, 1) and ball(3.0, (1.37, 1.37, 7.7)).shape == (5, 5, 1)
    assert ball(1.0).sum() == 7 and ball(3.0).sum() == 123


def test_distance_transform_host():
    from aide_amd.morphology import distance_transform
    for case in CASES:
        fg = case.volume != 0
        if fg.all():
            continue
        got = distance_transform(case.volume)
        assert got.dtype == np.float64 and got.flags['C_CONTIGUOUS']
        assert np.array_equal(got, mc.brute_distance(fg, mc.UNIT)), case.name                  # integers: bit-equal
        got, want = distance_transform(case.volume, mc.SPACING), mc.brute_distance(fg, mc.SPACING)
        assert np.all(np.abs(got - want) <= mc.REL * want), case.name
    vol = CLASS_CASES[2].volume
    assert np.array_equal(distance_transform(vol, cls=3), mc.brute_distance(vol == 3, mc.UNIT))
    full = np.ones((3, 4, 5), np.int64)
    got = distance_transform(full, mc.SPACING)
    assert got.shape == full.shape and np.all(np.isposinf(got))                                # no background voxel: +inf
    assert np.all(np.isposinf(distance_transform(full * 2, cls=2))) and not distance_transform(full * 2, cls=1).any()
    assert not distance_transform(np.zeros((3, 4, 5), np.uint8)).any()
    assert np.all(np.isposinf(mc.brute_distance(full != 0, mc.UNIT)))


def test_argument_validation():
    from aide_amd import morphology as m
    vol = CASES[2].volume
    for bad in (-1.0, float('nan'), float('inf'), None, '3', True):
        with pytest.raises(ValueError):
            m.open_(vol, bad)
        with pytest.raises(ValueError):
            m.ball(bad)
    for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, float('inf'), 1.0), (float('nan'), 1.0, 1.0), 2.0):
        with pytest.raises(ValueError):
            m.close(vol, 1.0, bad)
        with pytest.raises(ValueError):
            m.distance_transform(vol, bad)
        with pytest.raises(ValueError):
            m.ball(1.0, bad)
    for bad in (1, 9, 0, True, 2.0):
        with pytest.raises(ValueError):
            m.dilate(vol, 1.0, mc.UNIT, bad)
    for bad in (2, -1, None, True):
        with pytest.raises(ValueError):
            m.erode(vol, 1.0, outside=bad)
    with pytest.raises(ValueError):
        m.distance_transform(vol, cls=-1)
    with pytest.raises(RuntimeError):
        m.erode(vol[0], 1.0)
    with pytest.raises(RuntimeError):
        m.erode(vol.astype(np.float32), 1.0)


def test_abi_rejects_bad_arguments_before_any_launch():
    """the argument checks of the two entry points return before they touch a device: they run without one"""
    import ctypes
    from aide_amd.build import build
    build(verbose=False)
    from aide_amd._lib import lib
    assert lib.aide_morph3d_ws_bytes(2 ** 31) == 0 and lib.aide_edt3d_ws_bytes(2 ** 31) == 0
    assert lib.aide_morph3d_ws_bytes(1000) >= 14 * 1000 and lib.aide_edt3d_ws_bytes(1000) >= 13 * 1000
    assert lib.aide_morph3d_ws_bytes(1000) % 16 == 0 and lib.aide_edt3d_ws_bytes(1000) % 16 == 0
    good = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    p = 4096                                      # never dereferenced: every call below is rejected first

    def morph(d=(4, 4, 4), classes=0, op=3, r=1.0, sp=good, v=p, u8=1, out=p, ws=p):
        return lib.aide_morph3d(v, u8, *d, 16, 4, 1, classes, op, r, sp, out, ws, None)

    def edt(d=(4, 4, 4), sp=good, v=p, u8=1, dist=p, ws=p):
        return lib.aide_edt3d(v, u8, *d, 16, 4, 1, -1, sp, dist, ws, None)

    assert morph(d=(0, 4, 4)) == 0 and edt(d=(4, 0, 4)) == 0                  # an empty volume launches nothing
    for kw in (dict(classes=1), dict(classes=9), dict(classes=-2), dict(op=5), dict(op=-1), dict(r=-0.5),
               dict(r=float('nan')), dict(r=float('inf')), dict(sp=None), dict(v=None), dict(out=None), dict(ws=None),
               dict(ws=p + 8), dict(v=p + 4, u8=0), dict(u8=2), dict(d=(2048, 2048, 512)), dict(d=(-1, 4, 4)),
               dict(sp=(ctypes.c_double * 3)(1.0, 0.0, 1.0)), dict(sp=(ctypes.c_double * 3)(1.0, 1.0, float('inf'))),
               dict(sp=(ctypes.c_double * 3)(float('nan'), 1.0, 1.0)), dict(sp=(ctypes.c_double * 3)(1.0, -1.0, 1.0))):
        assert morph(**kw) == -1, kw
    for kw in (dict(sp=None), dict(v=None), dict(dist=None), dict(ws=None), dict(ws=p + 8), dict(dist=p + 4),
               dict(v=p + 4, u8=0), dict(u8=-1), dict(d=(2048, 2048, 512)),
               dict(sp=(ctypes.c_double * 3)(1.0, 0.0, 1.0)), dict(sp=(ctypes.c_double * 3)(1.0, 1.0, float('inf')))):
        assert edt(**kw) == -1, kw


def test_predict_case_spacing_needs_an_operation():
    from aide_amd.inference import predict_case
    with pytest.raises(TypeError):
        predict_case(None, None, spacing=(1.0, 1.0, 2.0))
