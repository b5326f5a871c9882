"""CPU: aide_amd/volumes.py, the one place where the 3-D volume operators check and marshal their arguments: what
`device_volume` widens and keeps, what it rejects, that strides survive it, how `as3d` lifts and flattens, what `classes` and
`spacing` accept and reject (the rules of the copies they replace, written out here), and that every public operator still
raises its own exception type for a bad num_classes."""
import numpy as np
import pytest
import torch

from aide_amd import volumes


@pytest.mark.parametrize('dtype', [torch.int64, torch.int32, torch.int16, torch.int8, torch.bool, torch.uint8])
def test_device_volume_widens_to_int64(dtype):
    x = torch.arange(24).reshape(2, 3, 4).remainder(2).to(dtype)
    v = volumes.device_volume(x, 'test')
    assert v.dtype == torch.int64 and v.shape == x.shape and torch.equal(v, x.to(torch.int64))
    if dtype == torch.int64:
        assert v.data_ptr() == x.data_ptr()
    kept = volumes.device_volume(x, 'test', keep_uint8=True)
    assert kept.dtype == (torch.uint8 if dtype == torch.uint8 else torch.int64)
    assert volumes.u8(kept) == int(dtype == torch.uint8) and volumes.u8(v) == 0
    if dtype == torch.uint8:
        assert kept.data_ptr() == x.data_ptr()


@pytest.mark.parametrize('bad', [torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, 4, 5, dtype=torch.int64),
                                 torch.zeros(2, 3, 4, dtype=torch.float32), torch.zeros(2, 3, 4, dtype=torch.float64),
                                 torch.zeros(1).to(torch.uint8).expand(2048, 2048, 512)],
                         ids=['2-D', '4-D', 'float32', 'float64', '2^31 voxels'])
def test_device_volume_rejects(bad):
    for keep in (False, True):
        with pytest.raises(RuntimeError):
            volumes.device_volume(bad, 'test', keep_uint8=keep)
    with pytest.raises(RuntimeError):
        volumes.volume_args(bad, 'test')


def test_device_volume_accepts_the_largest_volume():
    volumes.volume_args(torch.zeros(1).to(torch.uint8).expand(2048, 2048, 512)[:, :, 1:], 'test')        # 2^31 - 2^22 voxels
    assert volumes.MAX_VOX == 2 ** 31 - 1
    assert volumes.device_volume(torch.zeros(0, 4, 4, dtype=torch.int32), 'test').shape == (0, 4, 4)


@pytest.mark.parametrize('dtype', [torch.int64, torch.uint8])
def test_strides_survive(dtype):
    base = torch.arange(5 * 6 * 7).reshape(5, 6, 7).remainder(3).to(dtype)
    for view in (base.permute(1, 2, 0), base.transpose(0, 2), base[::2], base[:, 1::2, ::3]):
        assert not view.is_contiguous()
        v = volumes.device_volume(view, 'test', keep_uint8=True)
        assert v.stride() == view.stride() and v.shape == view.shape and v.data_ptr() == view.data_ptr()
        a, b = volumes.device_pair(view, view, 'test')
        assert a.stride() == view.stride() and b.data_ptr() == view.data_ptr()
    widened = volumes.device_volume(base.to(torch.int32).permute(1, 2, 0), 'test')                       # a dense permuted view
    assert widened.stride() == base.permute(1, 2, 0).stride() and torch.equal(widened, base.permute(1, 2, 0).to(torch.int64))


def test_as3d_lifts_and_flattens():
    one = torch.arange(5, dtype=torch.int32)
    assert volumes.as3d(one).shape == (1, 1, 5) and volumes.as3d(one).dtype == torch.int64
    two = torch.zeros(4, 5, dtype=torch.uint8)
    assert volumes.as3d(two).shape == (1, 4, 5) and volumes.as3d(two).dtype == torch.uint8
    three = torch.zeros(3, 4, 5, dtype=torch.int64).permute(2, 0, 1)
    assert volumes.as3d(three).stride() == three.stride()
    five = torch.arange(2 * 3 * 4 * 5 * 6).reshape(2, 3, 4, 5, 6)
    flat = volumes.as3d(five)
    assert flat.shape == (24, 5, 6) and torch.equal(flat, five.reshape(24, 5, 6))
    assert volumes.as3d(torch.zeros(2, 3, dtype=torch.bool)).dtype == torch.int64


def test_device_pair_checks():
    a = torch.zeros(4, 5, 6, dtype=torch.int64)
    p, t = volumes.device_pair(a, a.to(torch.uint8), 'test')
    assert p.dtype == torch.int64 and t.dtype == torch.uint8 and p.shape == t.shape == (4, 5, 6)
    p, t = volumes.device_pair(a[0, 0], a[0, 0].to(torch.int16), 'test')
    assert p.shape == t.shape == (1, 1, 6) and t.dtype == torch.int64
    big = torch.zeros(1).to(torch.uint8).expand(2 ** 31)
    scalar = torch.zeros((), dtype=torch.int64)
    for x, y in ((a, torch.zeros(4, 6, 5, dtype=torch.int64)), (a, a.float()), (a.double(), a), (scalar, scalar), (big, big)):
        with pytest.raises(RuntimeError):
            volumes.device_pair(x, y, 'test')


def test_host_volume():
    x = torch.arange(24, dtype=torch.int32).reshape(2, 3, 4)
    got = volumes.host_volume(x, 'test')
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, x.numpy())
    assert volumes.host_volume(x.numpy() > 3, 'test').dtype == np.bool_
    assert volumes.host_volume([[[1, 2]]], 'test').shape == (1, 1, 2)
    for bad in (x[0], x.float(), np.zeros((2, 3, 4, 5), np.int64), np.zeros((2, 3, 4), np.float64)):
        with pytest.raises(RuntimeError):
            volumes.host_volume(bad, 'test')


# num_classes -> what the strict rule (keep_components, fill_holes, label_components, lesion_*, erode / dilate / open_ / close)
# and the older rule (keep_largest_per_class, keep_largest_batched, case_scores, surface_scores, predict_case) make of it
CLASSES = [(None, None, TypeError), (2, 2, 2), (8, 8, 8), (1, ValueError, RuntimeError), (9, ValueError, RuntimeError),
           (True, ValueError, RuntimeError), (2.0, ValueError, 2), ('3', ValueError, 3), (np.int64(5), 5, 5)]


@pytest.mark.parametrize('value, strict, older', CLASSES, ids=[repr(c[0]) for c in CLASSES])
def test_classes(value, strict, older):
    for want, kw in ((strict, {}), (older, dict(strict=False))):
        if isinstance(want, type):
            with pytest.raises(want):
                volumes.classes(value, 'test', **kw)
        else:
            got = volumes.classes(value, 'test', **kw)
            assert got == want and (got is None or type(got) is int)


SPACINGS = [((1.0, 2.0), False), ((1.0, 0.0, 1.0), False), ((1.0, float('inf'), 1.0), False), ((1.0, 1.0, float('nan')), False),
            (1.5, False), ((1.0, -2.0, 1.0), False), ((1.0, 1.0, 1.0, 1.0), False), (None, False),
            ((1, 2.5, 0.5), True), ([0.7, 0.7, 5.5], True), (np.array([1.37, 1.37, 7.7]), True)]


@pytest.mark.parametrize('value, ok', SPACINGS, ids=[repr(s[0]) for s in SPACINGS])
def test_spacing(value, ok):
    if not ok:
        with pytest.raises(ValueError):
            volumes.spacing(value, 'test')
        return
    got = volumes.spacing(value, 'test')
    assert got == tuple(float(v) for v in value) and all(type(v) is float for v in got)


def test_workspace():
    like = torch.zeros(3, 4, 5, dtype=torch.int64)
    seen = []
    ws = volumes.workspace(lambda n, *a: seen.append((n,) + a) or 48, like, 7, 2)
    assert seen == [(60, 7, 2)] and ws.dtype == torch.uint8 and ws.shape == (48,) and ws.device == like.device


VOL = np.zeros((3, 4, 5), np.int64)


def _public():
    from aide_amd import inference as inf, morphology as m
    from aide_amd.utils import metrics3d
    return [('keep_largest_per_class', RuntimeError, lambda c: inf.keep_largest_per_class(VOL, c)),
            ('keep_largest_batched', RuntimeError, lambda c: inf.keep_largest_batched(VOL, [0, 3], num_classes=c)),
            ('keep_components', ValueError, lambda c: inf.keep_components(VOL, num_classes=c)),
            ('fill_holes', ValueError, lambda c: inf.fill_holes(VOL, c)),
            ('label_components', ValueError, lambda c: inf.label_components(VOL, c)),
            ('lesion_counts', ValueError, lambda c: inf.lesion_counts(VOL, VOL, c)),
            ('lesion_scores', ValueError, lambda c: inf.lesion_scores(VOL, VOL, c)),
            ('case_scores', RuntimeError, lambda c: inf.case_scores(VOL, VOL, num_classes=c)),
            ('predict_case', RuntimeError, lambda c: inf.predict_case(None, keep_largest='per_class', num_classes=c)),
            ('surface_scores', RuntimeError, lambda c: metrics3d.surface_scores(VOL, VOL, (1.0, 1.0, 1.0), c)),
            ('erode', ValueError, lambda c: m.erode(VOL, 1.0, num_classes=c)),
            ('dilate', ValueError, lambda c: m.dilate(VOL, 1.0, num_classes=c)),
            ('open_', ValueError, lambda c: m.open_(VOL, 1.0, num_classes=c)),
            ('close', ValueError, lambda c: m.close(VOL, 1.0, num_classes=c))]


PUBLIC = ('keep_largest_per_class', 'keep_largest_batched', 'keep_components', 'fill_holes', 'label_components', 'lesion_counts',
          'lesion_scores', 'case_scores', 'predict_case', 'surface_scores', 'erode', 'dilate', 'open_', 'close')


@pytest.mark.parametrize('index', range(len(PUBLIC)), ids=PUBLIC)
def test_public_functions_keep_their_exception_type(index):
    name, error, call = _public()[index]
    assert name == PUBLIC[index]
    for bad in (9, 1):
        with pytest.raises(error):
            call(bad)
    if name != 'predict_case':                     # (which would go on to the network)
        call(3)                                    # a good one passes
    if error is ValueError:                        # the strict rule: no float, no bool
        with pytest.raises(ValueError):
            call(3.0)
        with pytest.raises(ValueError):
            call(True)
