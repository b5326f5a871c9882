"""-m gpu: the per-class largest-component filter on the device (aide_amd/csrc/eval3d.hip, aide_keep_largest_cc3d_classes and
its batched form) equals the numpy path of aide_amd.inference.keep_largest_per_class byte for byte, volume and stats, on every
case of lcc_cases; test_lcc_classes_host.py holds that numpy path to an independent flood fill.  Everything is integer."""
import functools

import numpy as np
import pytest
import torch

import lcc_cases

pytestmark = pytest.mark.gpu

CASES = lcc_cases.cases()


@functools.lru_cache(maxsize=None)
def _host(index, dtype=np.int64):
    """the numpy path on case `index` cast to `dtype`, computed once: (cast volume, filtered volume, stats)"""
    from aide_amd.inference import keep_largest_per_class
    name, vol, c = CASES[index]
    vol = vol.astype(dtype)                       # keeps the strides of a view (order 'K')
    out, stats = keep_largest_per_class(vol, c, stats=True)
    out.flags.writeable = stats.flags.writeable = False
    return vol, out, stats


def _device(vol, dev):
    t = torch.from_numpy(vol).to(dev)
    if vol.flags['C_CONTIGUOUS']:
        assert t.is_contiguous()
    else:                                         # a view stays a view: the kernels get its strides
        assert t.stride() == tuple(s // vol.itemsize for s in vol.strides) and not t.is_contiguous()
    return t


def _check(index, dtype, dev):
    from aide_amd.inference import keep_largest_per_class
    name, _, c = CASES[index]
    vol, want, want_stats = _host(index, dtype)
    got, stats = keep_largest_per_class(_device(vol, dev), c, stats=True)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == vol.shape and got.is_contiguous()
    assert stats.is_cuda and stats.dtype == torch.int64 and tuple(stats.shape) == (c, 3)
    got, stats = got.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(got, want), (name, dtype, int((got != want).sum()))
    assert np.array_equal(stats, want_stats), (name, dtype, stats, want_stats)
    alone = keep_largest_per_class(_device(vol, dev), c)                  # the select kernel without the stats sums
    assert isinstance(alone, torch.Tensor) and np.array_equal(alone.cpu().numpy(), want), (name, dtype)


@pytest.mark.parametrize('index', range(len(CASES)), ids=[c[0] for c in CASES])
def test_device_equals_numpy_path(dev, index):
    _check(index, np.int64, dev)


@pytest.mark.parametrize('dtype', [np.int32, np.uint8], ids=['int32', 'uint8'])
def test_device_other_integer_inputs(dev, dtype):
    """narrower labels are widened on the device; as uint8 the out-of-range case holds 253 instead of -3"""
    for index in range(len(CASES)):
        _check(index, dtype, dev)


def test_empty_volume(dev):
    from aide_amd.inference import keep_largest_per_class
    out, stats = keep_largest_per_class(torch.zeros(0, 4, 4, dtype=torch.int64, device=dev), 5, stats=True)
    assert out.numel() == 0 and out.dtype == torch.uint8 and stats.cpu().tolist() == [[0, 0, 0]] * 5


def test_two_classes_equals_binary_device_filter(dev):
    from aide_amd.inference import keep_largest_per_class, keep_largest_connected_components
    binary = [i for i, (_, _, c) in enumerate(CASES) if c == 2]
    assert len(binary) >= 3
    for index in binary:
        t = _device(_host(index)[0], dev)
        assert torch.equal(keep_largest_per_class(t, 2), keep_largest_connected_components(t)), CASES[index][0]
    for t in (torch.zeros(5, 17, 33, dtype=torch.int64, device=dev), torch.ones(5, 17, 33, dtype=torch.int64, device=dev)):
        assert torch.equal(keep_largest_per_class(t, 2), keep_largest_connected_components(t))


def test_same_bytes_whatever_the_workspace_held(dev):
    """two calls through the C ABI on one workspace that is filled with 0xFF before each: stale control words, parents or
    areas would show (a fresh torch.empty may happen to be clean)"""
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    for name in ('ties', 'out of range', 'eight classes'):
        index = [c[0] for c in CASES].index(name)
        vol, want, want_stats = _host(index)
        c = CASES[index][2]
        t = _device(vol, dev)
        ws = torch.empty(lib.aide_lcc3d_classes_ws_bytes(t.numel(), c), device=dev, dtype=torch.uint8)
        runs = []
        for _ in range(2):
            ws.fill_(0xFF)
            out = torch.full(t.shape, 0xEE, device=dev, dtype=torch.uint8)
            stats = torch.full((c, 3), -1, device=dev, dtype=torch.int64)
            check(lib.aide_keep_largest_cc3d_classes(ptr(t), *t.shape, *t.stride(), c, ptr(out), ptr(stats), ptr(ws),
                                                     stream_ptr()), 'keep_largest_cc3d_classes')
            runs.append((out.cpu().numpy().tobytes(), stats.cpu().numpy().tobytes()))
        assert runs[0] == runs[1], name
        assert runs[0] == (want.tobytes(), want_stats.tobytes()), name


def test_same_bytes_whatever_the_workspace_held_binary_and_batched(dev):
    """the same through the other entries of the C ABI: a 7 x 20 x 37 volume through the binary filter, and cases of 5, 1
    and 6 slices at 20 x 37 through the binary and the per-class batched filter, each on a zeroed workspace and on one filled
    with 0xFF -- identical bytes, and those of the CPU function (binary) and of the flood fill (per class)"""
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    from aide_amd.inference import keep_largest_connected_components
    rng = np.random.RandomState(17)
    c, k, (h, w) = 4, 3, (20, 37)
    vol = np.where(rng.rand(7, h, w) < 0.55, rng.randint(1, c, (7, h, w)), 0).astype(np.int64)
    lab = np.where(rng.rand(12, h, w) < 0.55, rng.randint(1, c, (12, h, w)), 0).astype(np.int64)
    start = [0, 5, 6, 12]
    cases = [lab[a:b].transpose(1, 2, 0) for a, b in zip(start, start[1:])]
    want_binary = np.concatenate([keep_largest_connected_components(x).transpose(2, 0, 1) for x in cases])
    fills = [lcc_cases.flood_fill(x, c) for x in cases]
    want_classes = np.concatenate([f[0].transpose(2, 0, 1) for f in fills])
    want_stats = np.stack([f[1] for f in fills])
    t, tl = torch.from_numpy(vol).to(dev), torch.from_numpy(lab).to(dev)
    table = torch.tensor(start, dtype=torch.int64, device=dev)

    def single(ws, out, stats):
        return lib.aide_keep_largest_cc3d(ptr(t), *t.shape, *t.stride(), ptr(out), ptr(ws), stream_ptr())

    def batched(ws, out, stats):
        return lib.aide_keep_largest_cc3d_batched(ptr(tl), ptr(table), k, *tl.shape, ptr(out), ptr(ws), stream_ptr())

    def classes_batched(ws, out, stats):
        return lib.aide_keep_largest_cc3d_classes_batched(ptr(tl), ptr(table), k, *tl.shape, c, ptr(out), ptr(stats), ptr(ws),
                                                          stream_ptr())

    for call, src, size, want, stats_want in (
            (single, t, lib.aide_lcc3d_ws_bytes(t.numel()), keep_largest_connected_components(vol), None),
            (batched, tl, lib.aide_lcc3d_batched_ws_bytes(tl.numel(), k), want_binary, None),
            (classes_batched, tl, lib.aide_lcc3d_classes_batched_ws_bytes(tl.numel(), k, c), want_classes, want_stats)):
        ws = torch.empty(size, device=dev, dtype=torch.uint8)
        runs = []
        for fill in (0x00, 0xFF):
            ws.fill_(fill)
            out = torch.full(src.shape, 0xEE, device=dev, dtype=torch.uint8)
            stats = torch.full((k, c, 3), -1, device=dev, dtype=torch.int64)
            check(call(ws, out, stats), call.__name__)
            runs.append((out.cpu().numpy().tobytes(), stats.cpu().numpy().tobytes()))
        assert runs[0] == runs[1], call.__name__
        assert runs[0][0] == np.ascontiguousarray(want).astype(np.uint8).tobytes(), call.__name__
        if stats_want is not None:
            assert runs[0][1] == stats_want.tobytes(), call.__name__


def _ragged(dev):
    """[15, 17, 33] labels 0 .. 4 of four cases with S_k = 1, 5, 0 (empty, in the middle) and 9; the table on the device"""
    rng = np.random.RandomState(3)
    lab = np.where(rng.rand(15, 17, 33) < 0.6, rng.randint(1, 5, (15, 17, 33)), 0).astype(np.int64)
    lab[8, 3, 4] = 7                              # out of range for C = 5
    start = [0, 1, 6, 6, 15]
    return torch.from_numpy(lab).to(dev), torch.tensor(start, dtype=torch.int64, device=dev), start


def test_batched_equals_per_case_device_calls(dev):
    from aide_amd.inference import keep_largest_batched, keep_largest_per_class
    lab, table, start = _ragged(dev)
    out, stats = keep_largest_batched(lab, table, num_classes=5, stats=True)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == lab.shape
    assert stats.is_cuda and stats.dtype == torch.int64 and tuple(stats.shape) == (4, 5, 3)
    for k, (a, b) in enumerate(zip(start, start[1:])):
        if a == b:
            assert not stats[k].any().item()
            continue
        want, st = keep_largest_per_class(lab[a:b].permute(1, 2, 0), 5, stats=True)
        assert torch.equal(out[a:b].permute(1, 2, 0), want), k
        assert torch.equal(stats[k], st), (k, stats[k].tolist(), st.tolist())
    assert torch.equal(keep_largest_batched(lab, table, num_classes=5), out)
    # and the numpy path of the batched call
    host, host_stats = keep_largest_batched(lab.cpu().numpy(), start, num_classes=5, stats=True)
    assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(stats.cpu().numpy(), host_stats)


def test_batched_default_is_the_binary_filter(dev):
    from aide_amd.inference import keep_largest_batched, keep_largest_connected_components
    lab, table, start = _ragged(dev)
    out = keep_largest_batched(lab, table)
    assert out.dtype == torch.uint8 and int(out.max().item()) == 1
    for a, b in zip(start, start[1:]):
        if b > a:
            assert torch.equal(out[a:b].permute(1, 2, 0), keep_largest_connected_components(lab[a:b].permute(1, 2, 0)))


@pytest.mark.parametrize('name', ['UNet', 'fuseunet'])
def test_predict_case_per_class(dev, name):
    from aide_amd.inference import predict_case, keep_largest_per_class
    from aide_amd.models_singlemodalinput import UNet
    from aide_amd.models_twomodalinputs import fuseunet
    two = name == 'fuseunet'
    torch.manual_seed(5)
    net = fuseunet(5) if two else UNet(5)
    with torch.no_grad():                         # the default head is all bias at 32 x 32: every pixel would be class 0
        net.last_conv1.weight.normal_(0.0, 1.0)
        net.last_conv1.bias.zero_()
    net = net.to(dev)
    g = torch.Generator().manual_seed(77)
    net.train()
    with torch.no_grad():
        for _ in range(2):                        # running statistics that are not the initial (0, 1)
            net(*[torch.randn(4, 3, 32, 32, generator=g).to(dev) for _ in range(2 if two else 1)])
    net.eval()
    sl = [torch.randn(6, 3, 32, 32, generator=g).to(dev) for _ in range(2 if two else 1)]
    raw = predict_case(net, *sl, batch_size=4, numpy=False)
    assert raw.is_cuda and tuple(raw.shape) == (32, 32, 6) and len(torch.unique(raw)) > 2
    want = keep_largest_per_class(raw, 5)
    got = predict_case(net, *sl, batch_size=4, keep_largest='per_class', num_classes=5, numpy=False)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, want)
    host = keep_largest_per_class(raw.cpu().numpy(), 5)
    assert np.array_equal(got.cpu().numpy(), host)
    as_numpy = predict_case(net, *sl, batch_size=4, keep_largest='per_class', num_classes=5)
    assert isinstance(as_numpy, np.ndarray) and as_numpy.dtype == np.uint8 and np.array_equal(as_numpy, host)
    with pytest.raises(TypeError):
        predict_case(net, *sl, keep_largest='per_class')
