"""-m gpu: the case post-processing on the device (aide_amd/csrc/eval3d.hip, aide_keep_components3d and aide_fill_holes3d)
equals the flood fill of postprocess_cases byte for byte, volume and stats, on every case; every call is issued twice and must
give the same bytes; top_k = 1, min_voxels = 1 equals the two existing device filters.  Everything is integer."""
import numpy as np
import pytest
import torch

import postprocess_cases as pc

pytestmark = pytest.mark.gpu

CASES = pc.cases()
HOLES, COMPONENTS = CASES['holes'], CASES['components']


def _device(vol, dev):
    t = torch.from_numpy(np.array(vol, order='K', copy=True)).to(dev)
    if vol.flags['C_CONTIGUOUS']:
        assert t.is_contiguous()
    else:                                         # a view stays a view: the kernels get its strides
        assert t.stride() == tuple(s // vol.itemsize for s in vol.strides) and not t.is_contiguous()
    return t


def _twice(call):
    """(volume, stats) of a device call as numpy arrays, after a second call gave the same bytes"""
    runs = []
    for _ in range(2):
        out, stats = call()
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
        assert stats.is_cuda and stats.dtype == torch.int64
        runs.append((out.cpu().numpy(), stats.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    return runs[0]


@pytest.mark.parametrize('index', range(len(HOLES)), ids=[c.name for c in HOLES])
def test_fill_holes_device_equals_flood_fill(dev, index):
    from aide_amd.inference import fill_holes
    case = HOLES[index]
    t = _device(case.volume, dev)
    assert t.dtype == (torch.uint8 if case.volume.dtype == np.uint8 else torch.int64)
    before = t.clone()
    for axis in case.axes:
        want, want_stats, _ = pc.holes_reference(index, axis)
        got, stats = _twice(lambda: fill_holes(t, case.classes, axis, stats=True))
        assert got.shape == case.volume.shape and stats.shape == (case.classes or 2, 2)
        assert np.array_equal(got, want), (case.name, axis, int((got != want).sum()))
        assert np.array_equal(stats, want_stats), (case.name, axis, stats, want_stats)
        alone = fill_holes(t, case.classes, axis)
        assert isinstance(alone, torch.Tensor) and np.array_equal(alone.cpu().numpy(), want), (case.name, axis)
    assert torch.equal(t, before) and t.stride() == before.stride()


@pytest.mark.parametrize('index', range(len(COMPONENTS)), ids=[c.name for c in COMPONENTS])
def test_keep_components_device_equals_flood_fill(dev, index):
    from aide_amd.inference import keep_components
    case = COMPONENTS[index]
    t = _device(case.volume, dev)
    before = t.clone()
    want, want_stats = pc.components_reference(index)
    if case.classes is None:
        runs = [keep_components(t, case.top_k, case.min_voxels).cpu().numpy() for _ in range(2)]
        assert runs[0].dtype == np.uint8 and runs[0].tobytes() == runs[1].tobytes()
        assert np.array_equal(runs[0], want), (case.name, int((runs[0] != want).sum()))
    else:
        got, stats = _twice(lambda: keep_components(t, case.top_k, case.min_voxels, case.classes, stats=True))
        assert got.shape == case.volume.shape and stats.shape == (case.classes, 3)
        assert np.array_equal(got, want), (case.name, int((got != want).sum()))
        assert np.array_equal(stats, want_stats), (case.name, stats, want_stats)
        alone = keep_components(t, case.top_k, case.min_voxels, case.classes)             # the select pass without the stats sums
        assert isinstance(alone, torch.Tensor) and np.array_equal(alone.cpu().numpy(), want), case.name
    assert torch.equal(t, before) and t.stride() == before.stride()


def test_keep_components_defaults_equal_the_device_filters(dev):
    from aide_amd.inference import keep_components, keep_largest_connected_components, keep_largest_per_class
    volumes = {}
    for case in COMPONENTS:
        volumes.setdefault(case.volume.tobytes() + repr(case.volume.shape).encode(), (case.name, case.volume))
    assert len(volumes) >= 20
    for name, vol in volumes.values():
        t = _device(vol, dev)
        assert torch.equal(keep_components(t), keep_largest_connected_components(t)), name
        for c in (2, 5, 8):
            got, stats = keep_components(t, 1, 1, c, stats=True)
            want, want_stats = keep_largest_per_class(t, c, stats=True)
            assert torch.equal(got, want) and torch.equal(stats, want_stats), (name, c, stats.tolist(), want_stats.tolist())


def test_other_integer_inputs_and_empty_volumes(dev):
    """narrower labels are widened on the device (uint8 stays for fill_holes); an empty volume launches nothing"""
    from aide_amd.inference import keep_components, fill_holes
    names = {case.name: index for index, case in enumerate(HOLES)}
    index = names['blocky 7']
    t = _device(HOLES[index].volume, dev)
    for dtype in (torch.int32, torch.uint8, torch.int8):
        got, stats = fill_holes(t.to(dtype), 5, None, stats=True)
        assert np.array_equal(got.cpu().numpy(), pc.holes_reference(index, None)[0])
        assert np.array_equal(stats.cpu().numpy(), pc.holes_reference(index, None)[1])
    names = {case.name: index for index, case in enumerate(COMPONENTS)}
    index = names['ties per class']
    case = COMPONENTS[index]
    for dtype in (torch.int32, torch.uint8):
        got = keep_components(_device(case.volume, dev).to(dtype), case.top_k, case.min_voxels, case.classes)
        assert np.array_equal(got.cpu().numpy(), pc.components_reference(index)[0])
    empty = torch.zeros(0, 4, 4, dtype=torch.int64, device=dev)
    out, stats = keep_components(empty, 2, 1, 5, stats=True)
    assert out.numel() == 0 and out.dtype == torch.uint8 and stats.cpu().tolist() == [[0, 0, 0]] * 5
    out, stats = fill_holes(empty, 5, 2, stats=True)
    assert out.numel() == 0 and out.dtype == torch.uint8 and stats.cpu().tolist() == [[0, 0]] * 5


def test_same_bytes_whatever_the_workspace_held(dev):
    """through the C ABI on one workspace filled with 0x00 and with 0xFF before the call: stale control words, parents, areas or
    root words would show (a fresh torch.empty may happen to be clean)"""
    import ctypes
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    names = {case.name: index for index, case in enumerate(HOLES)}
    for name, axis in (('blocky 8', None), ('blocky 8', 2), ('uint8 classes', None), ('random binary 9x40x21 0.6', 0)):
        index = names[name]
        case = HOLES[index]
        want, want_stats, _ = pc.holes_reference(index, axis)
        t = _device(case.volume, dev)
        ws = torch.empty(lib.aide_fill_holes3d_ws_bytes(t.numel()), device=dev, dtype=torch.uint8)
        for fill in (0x00, 0xFF):
            ws.fill_(fill)
            out = torch.full(t.shape, 0xEE, device=dev, dtype=torch.uint8)
            stats = torch.full((case.classes or 2, 2), -1, device=dev, dtype=torch.int64)
            check(lib.aide_fill_holes3d(ptr(t), int(t.dtype == torch.uint8), *t.shape, *t.stride(), case.classes or 0,
                                        -1 if axis is None else axis, ptr(out), ptr(stats), ptr(ws), stream_ptr()), 'fill_holes3d')
            assert out.cpu().numpy().tobytes() == want.tobytes() and stats.cpu().numpy().tobytes() == want_stats.tobytes(), (name, fill)
    names = {case.name: index for index, case in enumerate(COMPONENTS)}
    for name in ('ties per class floor', 'eight classes', 'three blobs top 3'):
        index = names[name]
        case = COMPONENTS[index]
        want, want_stats = pc.components_reference(index)
        c = case.classes
        rows = c or 2
        ks = [0 if k is None else k for k in (case.top_k if isinstance(case.top_k, tuple) else [case.top_k] * rows)]
        ms = list(case.min_voxels) if isinstance(case.min_voxels, tuple) else [case.min_voxels] * rows
        ks, ms = (ks + [1] * 8)[:8], (ms + [1] * 8)[:8]
        t = _device(case.volume, dev)
        ws = torch.empty(lib.aide_components3d_ws_bytes(t.numel()), device=dev, dtype=torch.uint8)
        for fill in (0x00, 0xFF):
            ws.fill_(fill)
            out = torch.full(t.shape, 0xEE, device=dev, dtype=torch.uint8)
            stats = torch.full((rows, 3), -1, device=dev, dtype=torch.int64)
            check(lib.aide_keep_components3d(ptr(t), *t.shape, *t.stride(), c or 0, (ctypes.c_int * 8)(*ks),
                                             (ctypes.c_longlong * 8)(*ms), ptr(out), ptr(stats) if c else None, ptr(ws),
                                             stream_ptr()), 'keep_components3d')
            assert out.cpu().numpy().tobytes() == want.tobytes(), (name, fill)
            if c:
                assert stats.cpu().numpy().tobytes() == want_stats.tobytes(), (name, fill, stats.tolist())


def test_launch_counts(dev):
    """the kernel timer counts the launches themselves: 4 + max(1, top_k) for keep_components whatever the volume, the class
    count, min_voxels and stats are; five for fill_holes"""
    from aide_amd.profiling import DispatchTimer
    from aide_amd.inference import keep_components, fill_holes
    names = {case.name: index for index, case in enumerate(COMPONENTS)}

    def launches(call):
        torch.cuda.synchronize()
        timer = DispatchTimer(32, families=[15])  # family 15: the kernels of eval3d.hip (and other small ones)
        timer.start()
        try:
            call()
        finally:
            timer.stop()
        return len(timer.timeline())

    for name in ('all zero', 'eight classes', 'serpentine'):
        t = _device(COMPONENTS[names[name]].volume, dev)
        for top_k, want in ((None, 5), (1, 5), (2, 6), (3, 7), (8, 12)):
            assert launches(lambda: keep_components(t, top_k, 3)) == want, (name, top_k)
            assert launches(lambda: keep_components(t, top_k, 1, 8, stats=True)) == want, (name, top_k)
        assert launches(lambda: keep_components(t, (0, 1, 3, None, 2), (1, 9, 1, 1, 1), 5)) == 7, name
        for c, axis in ((None, None), (5, None), (8, 2), (None, 0)):
            assert launches(lambda: fill_holes(t, c, axis, stats=True)) == 5, (name, c, axis)
            assert launches(lambda: fill_holes(t.to(torch.uint8), c, axis)) == 5, (name, c, axis)


def test_fill_holes_of_the_filter_output(dev):
    """the uint8 output of the filters goes straight in: per class, and binary along the slice axis"""
    from aide_amd.inference import keep_components, fill_holes
    names = {case.name: index for index, case in enumerate(HOLES)}
    vol = HOLES[names['blocky 7']].volume
    t = _device(vol, dev)
    kept = keep_components(t, 2, 4, 5)
    host = keep_components(vol, 2, 4, 5)
    assert kept.dtype == torch.uint8 and np.array_equal(kept.cpu().numpy(), host)
    for c, axis in ((5, None), (5, 2), (None, 2)):
        got, stats = fill_holes(kept, c, axis, stats=True)
        want, want_stats, fate = pc.flood_holes(host, c, axis)
        assert fate['filled'] >= 1
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(stats.cpu().numpy(), want_stats), (c, axis)


@pytest.fixture(scope='module')
def tiny_case(dev):
    """a five-class UNet at 32 x 32 with a head that gives every class, six slices, and its unfiltered prediction"""
    from aide_amd.inference import predict_case
    from aide_amd.models_singlemodalinput import UNet
    torch.manual_seed(5)
    net = UNet(5)
    with torch.no_grad():                         # the default head is all bias at 32 x 32: every pixel would be class 0
        net.last_conv1.weight.normal_(0.0, 1.0)
        net.last_conv1.bias.zero_()
    net = net.to(dev)
    g = torch.Generator().manual_seed(77)
    net.train()
    with torch.no_grad():
        for _ in range(2):                        # running statistics that are not the initial (0, 1)
            net(torch.randn(4, 3, 32, 32, generator=g).to(dev))
    net.eval()
    slices = torch.randn(6, 3, 32, 32, generator=g).to(dev)
    raw = predict_case(net, slices, batch_size=4, numpy=False)
    assert raw.is_cuda and tuple(raw.shape) == (32, 32, 6) and len(torch.unique(raw)) > 2
    return net, slices, raw


def test_predict_case_new_arguments(dev, tiny_case):
    from aide_amd.inference import predict_case, keep_components, fill_holes
    net, slices, raw = tiny_case
    host = raw.cpu().numpy()
    got = predict_case(net, slices, batch_size=4, keep_largest='per_class', num_classes=5, top_k=(0, 1, 2, 3, None),
                       min_voxels=(1, 1, 2, 2, 3), fill_holes=True, slice_axis=2, numpy=False)
    by_hand = fill_holes(keep_components(raw, (0, 1, 2, 3, None), (1, 1, 2, 2, 3), 5), 5, 2)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, by_hand)
    want = pc.flood_holes(pc.flood_components(host, 5, (0, 1, 2, 3, None), (1, 1, 2, 2, 3))[0], 5, 2)[0]
    assert np.array_equal(got.cpu().numpy(), want)
    got = predict_case(net, slices, batch_size=4, keep_largest=True, top_k=3, fill_holes=True)
    want = pc.flood_holes(pc.flood_components(host, None, 3, 1)[0], None, None)[0]
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert torch.equal(predict_case(net, slices, batch_size=4, keep_largest=True, min_voxels=9, numpy=False),
                       keep_components(raw, 1, 9))
    assert torch.equal(predict_case(net, slices, batch_size=4, keep_largest=True, top_k=None, min_voxels=9, numpy=False),
                       keep_components(raw, None, 9))
    got = predict_case(net, slices, batch_size=4, fill_holes=True, slice_axis=2, numpy=False)      # no filter: binary
    assert torch.equal(got, fill_holes(raw, None, 2)) and np.array_equal(got.cpu().numpy(), pc.flood_holes(host, None, 2)[0])
    got = predict_case(net, slices, batch_size=4, fill_holes=True, num_classes=5, numpy=False)     # ... per class on request
    assert torch.equal(got, fill_holes(raw, 5)) and np.array_equal(got.cpu().numpy(), pc.flood_holes(host, 5, None)[0])
    with pytest.raises(TypeError):
        predict_case(net, slices, top_k=2)
    with pytest.raises(ValueError):
        predict_case(net, slices, keep_largest=True, top_k=9)


def test_predict_case_defaults_unchanged(dev, tiny_case):
    from aide_amd.inference import predict_case, keep_largest_connected_components, keep_largest_per_class
    net, slices, raw = tiny_case
    again = predict_case(net, slices, batch_size=4, numpy=False)
    assert again.dtype == torch.int64 and torch.equal(again, raw) and again.stride() == raw.stride()
    assert torch.equal(predict_case(net, slices, batch_size=4, keep_largest=True, numpy=False),
                       keep_largest_connected_components(raw))
    assert torch.equal(predict_case(net, slices, batch_size=4, keep_largest='per_class', num_classes=5, numpy=False),
                       keep_largest_per_class(raw, 5))
    as_numpy = predict_case(net, slices, batch_size=4)
    assert isinstance(as_numpy, np.ndarray) and as_numpy.dtype == np.int64 and np.array_equal(as_numpy, raw.cpu().numpy())


def test_full_size_case_equals_host_path(dev):
    """256 x 256 x 33 as predict_case lays it out (a permuted view of [S,H,W]): 2.2 million nodes, thousands of tiles and a
    multi-block grid in every launch.  The reference is the host path (scipy), which the host tests hold to the flood fill."""
    from aide_amd.inference import keep_components, fill_holes
    rng = np.random.RandomState(21)
    s, h, w = 33, 256, 256
    coarse = np.kron(rng.randint(1, 4, (3, 8, 8)), np.ones((11, 32, 32), np.int64))       # organs: blocks of classes 1 .. 3
    noise = rng.rand(s, h, w)
    lab = np.where(noise < 0.35, 0, coarse)
    lab[noise > 0.995] = 6                        # out of range for C = 5
    lab[:, 100:140, 100:140] = 2
    lab[5:28, 110:130, 110:130] = 0               # one large cavity across many tiles
    vol = lab.transpose(1, 2, 0)                  # [H,W,S], strides of [S,H,W]
    t = torch.from_numpy(lab).to(dev).permute(1, 2, 0)
    assert not t.is_contiguous() and tuple(t.shape) == (h, w, s)
    for axis in (None, 2):
        got, stats = fill_holes(t, 5, axis, stats=True)
        want, want_stats = fill_holes(vol, 5, axis, stats=True)
        assert want_stats[1:4, 0].min() > 100 and vol[120, 120, 16] == 0 and want[120, 120, 16] == 2
        assert np.array_equal(stats.cpu().numpy(), want_stats), (axis, stats.tolist(), want_stats.tolist())
        assert np.array_equal(got.cpu().numpy(), want), axis
    got = fill_holes(t, None, None)
    assert np.array_equal(got.cpu().numpy(), fill_holes(vol))
    got, stats = keep_components(t, (0, 1, 2, 8, None), (1, 1, 50, 2, 1), 5, stats=True)
    want, want_stats = keep_components(vol, (0, 1, 2, 8, None), (1, 1, 50, 2, 1), 5, stats=True)
    assert want_stats[1:4, 0].min() > 100 and (want_stats[1:4, 2] > 0).all()
    assert np.array_equal(stats.cpu().numpy(), want_stats), (stats.tolist(), want_stats.tolist())
    assert np.array_equal(got.cpu().numpy(), want)
    got = keep_components(t, 3, 5)
    assert np.array_equal(got.cpu().numpy(), keep_components(vol, 3, 5))
