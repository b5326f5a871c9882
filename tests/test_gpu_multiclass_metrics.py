"""-m gpu: the multi-class metrics on the device (aide_amd/csrc/metrics_mc.hip, aide_amd/utils/metrics2d.py, the per-class form
of aide_amd.inference.case_scores).  The four functions reproduce fixture g25 (the reference's own results) bit for bit, the
counts kernel equals a numpy statement of argmax + one-hot sums exactly over every target kind, the tails of the vector and
the scalar path, strided batches, NaN logits and ties, the meter equals the host loop over the concatenated images bit for
bit, and bad arguments raise before a launch.  Integer counts are exact and the float64 values are single IEEE operations in
a fixed order: nothing here has a tolerance."""
import os

import numpy as np
import pytest
import torch

from test_multiclass_metrics_host import CONF, GOLD, check_fixture, class_sums, host_loop, same_bits

pytestmark = pytest.mark.gpu

HWS = [(1, 1), (6, 10), (7, 9), (8, 8), (5, 13), (16, 16), (48, 80)]      # HW = 1, 60, 63, 64, 65, 256, 3840
KINDS = ['f32', 'i64', 'u8', 'index']


@pytest.fixture(scope='module')
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def numpy_counts(logits, index):
    """argmax (torch's rule on the host: ties -> lowest class, the first NaN wins) + one-hot sums"""
    n, c = logits.shape[:2]
    pred = torch.argmax(torch.from_numpy(logits), dim=1).numpy().reshape(n, -1)
    idx = index.reshape(n, -1)
    out = np.zeros((n, c, 3), np.int64)
    for k in range(c):
        i, t = pred == k, idx == k
        out[:, k, 0], out[:, k, 1], out[:, k, 2] = (i & t).sum(1), i.sum(1), t.sum(1)
    return out


def make(rng, n, c, h, w):
    x = rng.randn(n, c, h, w).astype(np.float32)
    x[rng.rand(n, c, h, w) < 0.2] = 0.5                        # many exact ties between classes
    return x, rng.randint(0, c, size=(n, h, w)).astype(np.int64)


def target_of(index, c, kind, dev):
    if kind == 'index':
        return torch.from_numpy(index).to(dev)
    onehot = index[:, None] == np.arange(c)[None, :, None, None]
    dt = {'f32': np.float32, 'i64': np.int64, 'u8': np.uint8}[kind]
    return torch.from_numpy(onehot.astype(dt)).to(dev)


@pytest.mark.parametrize('key', ['c2', 'c3', 'c5', 'c8', 'c5one'])
def test_fixture_device(gold, dev, key):
    check_fixture(gold, key, lambda x, t: (torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)))


def test_fixture_device_target_kinds(gold, dev):
    check_fixture(gold, 'c5', lambda x, t: (torch.from_numpy(x).to(dev), torch.from_numpy(t).float().to(dev)))
    check_fixture(gold, 'c8', lambda x, t: (torch.from_numpy(x).to(dev), torch.from_numpy(t).to(torch.uint8).to(dev)))
    check_fixture(gold, 'c3', lambda x, t: (torch.from_numpy(x).to(dev), torch.from_numpy(t.argmax(axis=1)).to(dev)))
    check_fixture(gold, 'c2', lambda x, t: (torch.from_numpy(x).to(dev), torch.from_numpy(t)))     # the target on the host


@pytest.mark.parametrize('c', [2, 3, 5, 8])
@pytest.mark.parametrize('kind', KINDS)
def test_counts_against_numpy(dev, c, kind):
    from aide_amd.utils import multiclass_counts
    rng = np.random.RandomState(10 * c + KINDS.index(kind))
    for n in (1, 3):
        for h, w in HWS:
            x, index = make(rng, n, c, h, w)
            got = multiclass_counts(torch.from_numpy(x).to(dev), target_of(index, c, kind, dev))
            assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (n, c, 3)
            assert np.array_equal(got.cpu().numpy(), numpy_counts(x, index)), (n, c, h, w, kind)


@pytest.mark.parametrize('kind', KINDS)
def test_counts_strided_batch(dev, kind):
    """logits and targets that are slices of larger tensors: a batch stride above C * HW, bases off the allocation's start
    (HW = 60: the base of image 1 is 16-byte aligned, the vector path; HW = 63: the scalar path)"""
    from aide_amd.utils import multiclass_counts
    rng = np.random.RandomState(5)
    for (h, w), c in (((6, 10), 5), ((7, 9), 3), ((16, 16), 8)):
        x, index = make(rng, 4, c + 2, h, w)
        big = torch.from_numpy(x).to(dev)
        view = big[1:, 1:1 + c]                                # batch stride (c + 2) * HW, channel offset HW
        assert not view.is_contiguous()
        idx = index[1:] % c
        tgt = target_of(index % c, c, kind, dev)[1:]
        got = multiclass_counts(view, tgt)
        assert np.array_equal(got.cpu().numpy(), numpy_counts(x[1:, 1:1 + c].copy(), idx)), (h, w, c, kind)
        every_other = torch.from_numpy(x).to(dev)[::2, :c]
        got = multiclass_counts(every_other, target_of(index % c, c, kind, dev)[::2])
        assert np.array_equal(got.cpu().numpy(), numpy_counts(x[::2, :c].copy(), (index % c)[::2])), (h, w, c, kind)


@pytest.mark.parametrize('c', [2, 3, 5, 8])
def test_counts_nan_ties_and_foreign_index(dev, c):
    from aide_amd.utils import multiclass_counts
    rng = np.random.RandomState(c)
    for h, w in ((6, 10), (16, 16)):
        x, index = make(rng, 3, c, h, w)
        x[0, c - 1, 1, 2] = np.nan                             # one NaN
        x[1, 0, 2, 3] = np.nan                                 # two NaNs in different classes: the first wins
        x[1, c - 1, 2, 3] = np.nan
        x[2, 1:, 3, 4] = np.nan                                # every class but 0
        x[2, :, 0, 0] = -np.inf                                # all equal
        index[0, 1, 2] = 255                                   # belongs to no class; the pixel is still predicted
        index[2, 0, 1] = -1
        index[2, 0, 2] = c
        want = numpy_counts(x, index)
        assert want[:, :, 1].sum() == 3 * h * w and want[:, :, 2].sum() == 3 * h * w - 3
        got = multiclass_counts(torch.from_numpy(x).to(dev), torch.from_numpy(index).to(dev))
        assert np.array_equal(got.cpu().numpy(), want), (c, h, w)
    zeros = torch.zeros(2, c, 16, 16, device=dev)              # whole-tensor ties: everything is class 0
    got = multiclass_counts(zeros, torch.zeros(2, 16, 16, dtype=torch.int64, device=dev)).cpu().numpy()
    assert (got[:, 0] == 256).all() and (got[:, 1:] == 0).all()


def test_counts_repeatable(dev):
    from aide_amd.utils import multiclass_counts
    rng = np.random.RandomState(8)
    x, index = make(rng, 3, 5, 48, 80)
    xd, td = torch.from_numpy(x).to(dev), target_of(index, 5, 'i64', dev)
    a = multiclass_counts(xd, td).cpu().numpy().tobytes()
    b = multiclass_counts(xd, td).cpu().numpy().tobytes()
    assert a == b


def test_meter(dev):
    """three updates with different N == the host loop over the concatenated images, float64 sums included"""
    from aide_amd.utils import MulticlassMeter
    rng = np.random.RandomState(12)
    c, h, w = 5, 6, 10
    x, index = make(rng, 7, c, h, w)
    x[:, 4] = -9.0
    index[index == 4] = 0                                      # a class in no image: unions of 0
    index[3] = 0
    meter = MulticlassMeter(c, dev)
    xd, td = torch.from_numpy(x).to(dev), torch.from_numpy(index).to(dev)
    for a, b in ((0, 1), (1, 4), (4, 7)):
        assert meter.update(xd[a:b], td[a:b]) is None
    got, want = meter.compute(), host_loop(x, index, h * w)
    assert got['images'] == 7
    for k in ('dice', 'iou') + CONF:
        assert same_bits(got[k], want[k]), (k, got[k], want[k])
    meter.reset()
    assert meter.compute()['images'] == 0
    meter.update(xd[:2], target_of(index[:2], c, 'u8', dev))
    got, want = meter.compute(), host_loop(x[:2], index[:2], h * w)
    for k in ('dice', 'iou') + CONF:
        assert same_bits(got[k], want[k]), (k, got[k], want[k])


def test_no_host_synchronisation(dev):
    """counts and meter updates complete with synchronising calls forbidden; compute() is the one copy"""
    from aide_amd.utils import MulticlassMeter, multiclass_counts
    rng = np.random.RandomState(4)
    x, index = make(rng, 3, 5, 16, 16)
    xd, td, oh = torch.from_numpy(x).to(dev), torch.from_numpy(index).to(dev), target_of(index, 5, 'i64', dev)
    meter = MulticlassMeter(5, dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        cnt = multiclass_counts(xd, oh)
        assert meter.update(xd, td) is None
        assert meter.update(xd[1:], oh[1:]) is None
        with pytest.raises(RuntimeError):
            meter.compute()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert cnt.is_cuda and meter.compute()['images'] == 5
    assert np.array_equal(cnt.cpu().numpy(), numpy_counts(x, index))


@pytest.mark.parametrize('dtype', [torch.int64, torch.uint8])
def test_case_scores_per_class(dev, dtype):
    from aide_amd.inference import case_scores
    rng = np.random.RandomState(21)
    for shape, c in (((16, 16, 5), 5), ((7, 9, 3), 3), ((7, 9, 3), 8)):
        p = rng.randint(0, c + 2, size=shape).astype(np.int64)             # labels >= C present in the prediction
        t = rng.randint(0, c, size=shape).astype(np.int64)
        want = class_sums(p, t, c)
        pd, td = torch.from_numpy(p).to(dev).to(dtype), torch.from_numpy(t).to(dev).to(dtype)
        got = case_scores(pd, td, num_classes=c)
        for k in want:
            assert same_bits(got[k], want[k]), (shape, c, k, got[k], want[k])
        # the [S,H,W] label maps of the inference loop as a permute(1, 2, 0) view, against an int64 target
        shw = torch.from_numpy(np.ascontiguousarray(p.transpose(2, 0, 1))).to(dev).to(dtype)
        view = shw.permute(1, 2, 0)
        assert not view.is_contiguous()
        got = case_scores(view, torch.from_numpy(t).to(dev), num_classes=c)
        for k in want:
            assert same_bits(got[k], want[k]), (shape, c, k, got[k], want[k])
    plain = case_scores((pd > 0).to(dtype), (td > 0).to(dtype))
    assert sorted(plain) == ['Dice', 'FN', 'FP', 'IoU', 'TN', 'TP'] and isinstance(plain['TP'], int)


def test_argument_errors_before_launch(dev):
    from aide_amd import utils as U
    from aide_amd.inference import case_scores
    from aide_amd._lib import lib
    z = lambda *s, **k: torch.zeros(*s, device=dev, **k)
    bad = [(z(1, 1, 4, 4), z(1, 1, 4, 4)), (z(1, 9, 4, 4), z(1, 9, 4, 4)), (z(1, 3, 4, 4, dtype=torch.float16), z(1, 3, 4, 4)),
           (z(2, 3, 4, 4), z(2, 3, 4, 5)), (z(2, 3, 4, 4), z(1, 4, 4, dtype=torch.int64)), (z(2, 3, 4, 4), z(2, 4, 4))]
    torch.cuda.synchronize()
    for x, t in bad:
        for fn in (U.multiclass_counts, U.MulticlassDice_fn, U.MulticlassIoU_fn, U.MulticlassTP_TN_FP_FN,
                   U.MulticlassAccuracy_fn):
            with pytest.raises(RuntimeError):
                fn(x, t)
    with pytest.raises(RuntimeError):
        U.MulticlassMeter(9, dev)
    with pytest.raises(RuntimeError):
        U.MulticlassMeter(5, dev).update(z(1, 3, 4, 4), z(1, 4, 4, dtype=torch.int64))
    for c in (1, 9):
        with pytest.raises(RuntimeError):
            case_scores(z(4, 4, 2, dtype=torch.int64), z(4, 4, 2, dtype=torch.int64), num_classes=c)
    with pytest.raises(RuntimeError):
        case_scores(z(4, 4, 2, dtype=torch.int64), z(4, 4, 3, dtype=torch.int64), num_classes=3)
    # the C ABI itself: AIDE_ERR_ARG (-1), nothing launched
    x, t, out = z(1, 8, 4, 4), z(1, 4, 4, dtype=torch.int64), z(8, 3, dtype=torch.int64)
    p = lambda v: v.data_ptr()
    assert lib.aide_mc_counts_logits(p(x), 128, p(t), 3, 16, 1, 1, 16, p(out), None) == -1
    assert lib.aide_mc_counts_logits(p(x), 128, p(t), 3, 16, 9, 1, 16, p(out), None) == -1
    assert lib.aide_mc_counts_logits(p(x), 128, p(t), 4, 16, 8, 1, 16, p(out), None) == -1
    assert lib.aide_mc_counts_logits(p(x), 16, p(t), 3, 16, 2, 2, 16, p(out), None) == -1       # overlapping images
    assert lib.aide_mc_counts_labels(p(t), 0, 16, 4, 1, p(t), 0, 16, 4, 1, 1, 4, 4, 9, p(out), None) == -1
    assert lib.aide_mc_counts_labels(p(t), 2, 16, 4, 1, p(t), 0, 16, 4, 1, 1, 4, 4, 3, p(out), None) == -1
    assert lib.aide_mc_metrics_accumulate(p(out), 1, 9, 16, p(out), None) == -1
    assert lib.aide_mc_metrics_accumulate(p(out), 1, 3, 16, None, None) == -1
    torch.cuda.synchronize()
