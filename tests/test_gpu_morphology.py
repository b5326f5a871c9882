"""-m gpu: ball morphology and the distance transform on the device (aide_amd/csrc/morph3d.hip, aide_morph3d; surface3d.hip,
aide_edt3d) against the brute force of morphology_cases, byte for byte: every operation, the radii with exact ties at unit
spacing and the tie-free radii at an anisotropic one, windows beyond the line length and windows of zero; the distance map
bit-equal to scipy at unit spacing and within the derived ulp bound otherwise; the multi-class rule; layouts; the same bytes
whatever the workspace held; `predict_case`'s new arguments."""
import ctypes

import numpy as np
import pytest
import torch

import morphology_cases as mc

pytestmark = pytest.mark.gpu

CASES, CLASS_CASES = mc.cases(), mc.class_cases()


def _call(vol, op, r, sp, classes=None):
    from aide_amd import morphology as m
    if op == 'erode0':
        return m.erode(vol, r, sp, classes, outside=0)
    if op == 'erode1':
        return m.erode(vol, r, sp, classes, outside=1)
    return {'dilate': m.dilate, 'open': m.open_, 'close': m.close}[op](vol, r, sp, classes)


def test_windows_of_the_settings_cover_both_extremes():
    """a condition on the chosen inputs: some window exceeds a line, some window is zero"""
    from aide_amd.morphology import ball
    assert ball(5.5, mc.SPACING).shape == (13, 9, 5) and ball(1.0, mc.SPACING).shape == (3, 1, 1)
    assert any(6 > c.volume.shape[0] for c in CASES) and any(4 > c.volume.shape[1] for c in CASES)
    assert any(3 > c.volume.shape[2] for c in CASES)


@pytest.mark.parametrize('index', range(len(CASES)), ids=[c.name for c in CASES])
def test_device_equals_brute_force(dev, index):
    case = CASES[index]
    t = torch.from_numpy(case.volume).to(dev)
    before = t.clone()
    for setting, (sp, r) in enumerate(mc.SETTINGS):
        for op in mc.OPS:
            got = _call(t, op, r, sp)
            assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and got.shape == t.shape
            got, want = got.cpu().numpy(), mc.reference('binary', index, op, setting)
            assert np.array_equal(got, want), (case.name, op, sp, r, int((got != want).sum()))
    assert torch.equal(t, before)


@pytest.mark.parametrize('index', range(len(CLASS_CASES)), ids=[c.name for c in CLASS_CASES])
def test_classes_equal_brute_force(dev, index):
    case = CLASS_CASES[index]
    t = torch.from_numpy(case.volume).to(dev)
    inrange = (case.volume >= 1) & (case.volume < case.classes)
    assert (case.volume[~inrange] != 0).any() or index == 0              # out-of-range values are present
    for setting, (sp, r) in enumerate(mc.SETTINGS):
        for op in mc.OPS:
            got = _call(t, op, r, sp, case.classes).cpu().numpy()
            want = mc.reference('classes', index, op, setting)
            assert np.array_equal(got, want), (case.name, op, sp, r, int((got != want).sum()))
            assert got.max() < case.classes                              # out-of-range values are written as 0 (or claimed)
            if op in ('dilate', 'close'):
                assert np.array_equal(got[inrange], case.volume[inrange]), (case.name, op, sp, r)   # never overwritten
    sp, r = mc.SETTINGS[3]
    reached = mc.brute_plane(inrange, 'dilate', r, sp)                   # by at least one class: the dilation of the union
    contested = int((reached & (mc.reference('classes', index, 'dilate', 3) == 0)).sum())
    assert contested > 0                          # reached and still 0: several classes claim the voxel


def test_contested_voxel_and_two_classes_as_binary(dev):
    vol = CLASS_CASES[0].volume                   # classes 1 and 2 with row 7 between them
    t = torch.from_numpy(vol).to(dev)
    got = _call(t, 'dilate', 1.0, mc.UNIT, 3).cpu().numpy()
    assert (got[:, 7, 3:13] == 0).all() and (got[:, 1, 3:13] == 1).all() and (got[:, 14, 3:13] == 2).all()
    for case in CASES:
        t = torch.from_numpy((case.volume != 0).astype(np.int64)).to(dev)           # a {0, 1} volume
        for op in mc.OPS:
            for sp, r in ((mc.UNIT, 2.0), (mc.SPACING, 3.3)):
                assert torch.equal(_call(t, op, r, sp, 2), _call(t, op, r, sp)), (case.name, op, sp, r)


def test_distance_transform(dev):
    from scipy import ndimage
    from aide_amd.morphology import distance_transform
    for case in CASES + CLASS_CASES:
        for cls in (None,) if case.classes is None else (None, 1, case.classes - 1):
            fg = (case.volume != 0) if cls is None else (case.volume == cls)
            if fg.all():
                continue
            for dtype in (np.int64, np.uint8):
                if dtype == np.uint8 and case.volume.min() < 0:
                    continue
                t = torch.from_numpy(case.volume.astype(dtype)).to(dev)
                got = distance_transform(t, cls=cls)
                assert got.is_cuda and got.dtype == torch.float64 and got.is_contiguous() and got.shape == t.shape
                want = ndimage.distance_transform_edt(fg)
                assert np.array_equal(got.cpu().numpy(), want), (case.name, cls)                   # integers: bit-equal
                got = distance_transform(t, mc.SPACING, cls).cpu().numpy()
                want = ndimage.distance_transform_edt(fg, sampling=mc.SPACING)
                err = np.abs(got - want)
                assert np.all(err <= mc.REL * want), (case.name, cls, float((err / np.maximum(want, 1e-300)).max()))
                assert np.array_equal(got == 0.0, ~fg)
    full = torch.ones(5, 17, 33, dtype=torch.int64, device=dev)
    assert torch.isposinf(distance_transform(full, mc.SPACING)).all()                              # no background voxel
    assert torch.isposinf(distance_transform(full * 3, cls=3)).all()
    assert not distance_transform(full * 3, cls=2).any() and not distance_transform(full * 0).any()
    assert distance_transform(torch.zeros(0, 4, 4, dtype=torch.int64, device=dev)).shape == (0, 4, 4)


@pytest.mark.parametrize('shape', mc.EDGE_SHAPES, ids=['%dx%dx%d' % s for s in mc.EDGE_SHAPES])
def test_distance_transform_chunk_and_workgroup_edges(dev, shape):
    """line lengths around the chunk of 32 and column counts around the workgroup of 64 of the walk the distance transform shares
    with the surface scores (surface_cases.EDGE_SHAPES) against the host path (scipy): int64 and uint8, a permuted view, every
    voxel a candidate (all background) and no candidate at all (all foreground: +inf)"""
    from aide_amd.morphology import distance_transform
    for density in (0.6, 0.97):
        vol = (np.random.RandomState(shape[0] + 3 * shape[1] + int(100 * density)).rand(*shape) < density).astype(np.int64)
        vol.flat[0] = 0                                                  # at least one background voxel
        unit, mm = distance_transform(vol), distance_transform(vol, mc.SPACING)
        assert np.array_equal(unit == 0.0, vol == 0) and np.isfinite(mm).all()
        view = torch.from_numpy(np.ascontiguousarray(vol.transpose(2, 0, 1))).to(dev).permute(1, 2, 0)   # [S,H,W] storage
        for t in (torch.from_numpy(vol).to(dev), torch.from_numpy(vol.astype(np.uint8)).to(dev), view):
            assert tuple(t.shape) == shape
            assert np.array_equal(distance_transform(t).cpu().numpy(), unit), (shape, density, t.dtype)   # integers: bit-equal
            got = distance_transform(t, mc.SPACING).cpu().numpy()
            assert np.all(np.abs(got - mm) <= mc.REL * mm), (shape, density, t.dtype)
            assert np.array_equal(got == 0.0, vol == 0)
    for dtype in (torch.int64, torch.uint8):
        full = torch.ones(shape, dtype=dtype, device=dev)
        assert torch.isposinf(distance_transform(full, mc.SPACING)).all() and np.isposinf(distance_transform(full.cpu().numpy())).all()
        assert not distance_transform(full * 0, mc.SPACING).any()


def test_layouts_and_types(dev):
    """int64 and uint8, contiguous and as the permute(1, 2, 0) view of [S,H,W] that predict_case produces: the same bytes"""
    from aide_amd.morphology import distance_transform
    for kind, index, classes in (('binary', 3, None), ('binary', 7, None), ('classes', 2, 5)):
        case = (CASES if kind == 'binary' else CLASS_CASES)[index]
        vol = np.where(case.volume < 0, 7, case.volume)                  # uint8 has no -1: another out-of-range value
        for setting in (4, 7):
            sp, r = mc.SETTINGS[setting]
            want = {op: mc.brute(vol, op, r, sp, classes) for op in ('open', 'close')}
            dist = None
            for dtype in (torch.int64, torch.uint8, torch.int32):
                c = torch.from_numpy(vol).to(dev).to(dtype)
                view = c.permute(2, 0, 1).contiguous().permute(1, 2, 0)  # [S,H,W] storage
                assert not view.is_contiguous() and torch.equal(view, c)
                for t in (c, view):
                    for op in ('open', 'close'):
                        got = _call(t, op, r, sp, classes)
                        assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), want[op]), (case.name, op, dtype)
                    d = distance_transform(t, sp)
                    assert d.is_contiguous() and (dist is None or torch.equal(d, dist))
                    dist = d
    empty = torch.zeros(4, 0, 4, dtype=torch.int64, device=dev)
    assert _call(empty, 'open', 2.0, mc.UNIT, 5).shape == (4, 0, 4)


def test_same_bytes_whatever_the_workspace_held(dev):
    """through the C ABI on one workspace filled with 0x00 and with 0xA5 before the call"""
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    from aide_amd.morphology import OPS
    for kind, index in (('binary', 3), ('binary', 5), ('classes', 2)):
        case = (CASES if kind == 'binary' else CLASS_CASES)[index]
        t = torch.from_numpy(case.volume).to(dev)
        ws = torch.empty(lib.aide_morph3d_ws_bytes(t.numel()), device=dev, dtype=torch.uint8)
        wd = torch.empty(lib.aide_edt3d_ws_bytes(t.numel()), device=dev, dtype=torch.uint8)
        for setting in (3, 8):
            sp, r = mc.SETTINGS[setting]
            spacing = (ctypes.c_double * 3)(*sp)
            for op in mc.OPS:
                runs = []
                for fill in (0x00, 0xA5):
                    ws.fill_(fill)
                    out = torch.full(t.shape, 0xEE, device=dev, dtype=torch.uint8)
                    check(lib.aide_morph3d(ptr(t), 0, *t.shape, *t.stride(), case.classes or 0, OPS[op], r, spacing, ptr(out),
                                           ptr(ws), stream_ptr()), 'morph3d')
                    runs.append(out.cpu().numpy())
                assert runs[0].tobytes() == runs[1].tobytes(), (case.name, op, sp, r)
                assert np.array_equal(runs[0], mc.reference(kind, index, op, setting)), (case.name, op, sp, r)
            runs = []
            for fill in (0x00, 0xA5):
                wd.fill_(fill)
                dist = torch.full(t.shape, -7.0, device=dev, dtype=torch.float64)
                check(lib.aide_edt3d(ptr(t), 0, *t.shape, *t.stride(), -1, spacing, ptr(dist), ptr(wd), stream_ptr()), 'edt3d')
                runs.append(dist.cpu().numpy())
            assert runs[0].tobytes() == runs[1].tobytes(), (case.name, sp)


def test_launch_counts(dev):
    """1 + 3 per class for erode / dilate, 1 + 6 per class for open / close, four for the distance transform, whatever the
    volume and the radius are"""
    from aide_amd.profiling import DispatchTimer
    from aide_amd.morphology import distance_transform

    def launches(call):
        torch.cuda.synchronize()
        timer = DispatchTimer(64, families=[15])
        timer.start()
        try:
            call()
        finally:
            timer.stop()
        return len(timer.timeline())

    for case in (CASES[3], CASES[0], CLASS_CASES[2]):
        t = torch.from_numpy(case.volume).to(dev)
        for sp, r in ((mc.UNIT, 0.0), (mc.SPACING, 5.5)):
            for op, per in (('erode0', 3), ('erode1', 3), ('dilate', 3), ('open', 6), ('close', 6)):
                assert launches(lambda: _call(t, op, r, sp)) == 1 + per, (case.name, op)
                assert launches(lambda: _call(t, op, r, sp, 5)) == 1 + 4 * per, (case.name, op)
            assert launches(lambda: distance_transform(t, sp)) == 4, case.name


@pytest.fixture(scope='module')
def tiny_case(dev):
    """a five-class UNet at 32 x 32 with a head that gives every class, six slices, and its unfiltered prediction (the network
    of test_gpu_postprocess.py)"""
    from aide_amd.inference import predict_case
    from aide_amd.models_singlemodalinput import UNet
    torch.manual_seed(5)
    net = UNet(5)
    with torch.no_grad():
        net.last_conv1.weight.normal_(0.0, 1.0)
        net.last_conv1.bias.zero_()
    net = net.to(dev)
    g = torch.Generator().manual_seed(77)
    net.train()
    with torch.no_grad():
        for _ in range(2):
            net(torch.randn(4, 3, 32, 32, generator=g).to(dev))
    net.eval()
    slices = torch.randn(6, 3, 32, 32, generator=g).to(dev)
    raw = predict_case(net, slices, batch_size=4, numpy=False)
    assert raw.is_cuda and tuple(raw.shape) == (32, 32, 6) and len(torch.unique(raw)) > 2
    return net, slices, raw


def test_predict_case_opening_closing(dev, tiny_case):
    from aide_amd.inference import (predict_case, keep_components, keep_largest_connected_components, keep_largest_per_class,
                                    fill_holes)
    from aide_amd.morphology import open_, close
    net, slices, raw = tiny_case
    host = raw.cpu().numpy()
    sp = (1.37, 1.37, 7.7)
    got = predict_case(net, slices, batch_size=4, opening=1.5, closing=3.0, spacing=sp, keep_largest='per_class', num_classes=5,
                       fill_holes=True, slice_axis=2, numpy=False)
    by_hand = close(fill_holes(keep_largest_per_class(open_(raw, 1.5, sp, 5), 5), 5, 2), 3.0, sp, 5)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, by_hand)
    opened = mc.brute(host, 'open', 1.5, sp, 5)
    assert np.array_equal(open_(raw, 1.5, sp, 5).cpu().numpy(), opened) and 0 < (opened != 0).sum() < (host != 0).sum()
    got = predict_case(net, slices, batch_size=4, opening=1.0, keep_largest=True, top_k=2, numpy=False)      # binary, unit spacing
    assert torch.equal(got, keep_components(open_(raw, 1.0), 2, 1))
    assert np.array_equal(open_(raw, 1.0).cpu().numpy(), mc.brute(host, 'open', 1.0, mc.UNIT))
    got = predict_case(net, slices, batch_size=4, closing=2.0, spacing=sp, keep_largest=True)
    want = close(keep_largest_connected_components(raw), 2.0, sp)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want.cpu().numpy())
    assert np.array_equal(got, mc.brute(keep_largest_connected_components(raw).cpu().numpy(), 'close', 2.0, sp))
    got = predict_case(net, slices, batch_size=4, opening=1.5, closing=1.5, spacing=sp, num_classes=5, numpy=False)   # no filter
    assert torch.equal(got, close(open_(raw, 1.5, sp, 5), 1.5, sp, 5))
    got = predict_case(net, slices, batch_size=4, closing=1.5, spacing=sp, numpy=False)                       # ... binary
    assert torch.equal(got, close(raw, 1.5, sp))
    with pytest.raises(TypeError):
        predict_case(net, slices, spacing=sp)
    with pytest.raises(ValueError):
        predict_case(net, slices, opening=-1.0)
    again = predict_case(net, slices, batch_size=4, numpy=False)         # without them: the call as it was
    assert again.dtype == torch.int64 and torch.equal(again, raw) and again.stride() == raw.stride()
    assert torch.equal(predict_case(net, slices, batch_size=4, keep_largest='per_class', num_classes=5, fill_holes=True,
                                    numpy=False), fill_holes(keep_largest_per_class(raw, 5), 5))
