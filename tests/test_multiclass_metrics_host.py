"""The multi-class metrics of aide_amd.utils without a GPU: the re-export list of the reference's utils/__init__.py:4-5, the
CPU path against fixture g25 (the reference's own results, tools/gen_golden_multiclass_metrics.py) bit for bit -- integer
counts are exact and every float64 value is the same IEEE operation sequence, so nothing here has a tolerance --, the
Accuracy restriction, index targets, the meter on the host, and the per-class form of inference.case_scores."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'g25_multiclass_metrics.npz')
CONF = ('TP', 'TN', 'FP', 'FN')


@pytest.fixture(scope='module')
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_reference_import_list():
    """the names of utils/__init__.py:4-5, as the train scripts import them"""
    from aide_amd.utils import Dice_fn, IoU_fn, TP_TN_FP_FN,  MulticlassDice_fn, MulticlassIoU_fn, MulticlassTP_TN_FP_FN,\
        MulticlassAccuracy_fn, Dice_fn_Nozero  # noqa: F401
    from aide_amd.utils import one_hot_result, multiclass_counts, MulticlassMeter  # noqa: F401


def check_fixture(gold, key, convert):
    """all four functions in both modes against the stored results; `convert(logits, onehot)` -> the arguments"""
    from aide_amd import utils as U
    c = gold[key + '/logits'].shape[1]
    for m, mode in enumerate(gold['modes'].tolist()):
        x, t = convert(gold[key + '/logits'], gold[key + '/onehot'])
        pre = '%s/m%d/' % (key, m)
        dice = U.MulticlassDice_fn(x, t, mode)
        iou = U.MulticlassIoU_fn(x, t, mode)
        conf = U.MulticlassTP_TN_FP_FN(x, t, mode)
        assert same_bits(dice, gold[pre + 'dice']), (key, mode, dice, gold[pre + 'dice'])
        assert same_bits(iou, gold[pre + 'iou']), (key, mode, iou, gold[pre + 'iou'])
        assert isinstance(conf, tuple) and len(conf) == 4
        for name, v in zip(CONF, conf):
            assert same_bits(v, gold[pre + name]), (key, mode, name, v, gold[pre + name])
        if c == 5:
            acc = U.MulticlassAccuracy_fn(x, t, mode)
            assert isinstance(acc, np.float64) and same_bits(acc, gold[pre + 'accuracy']), (key, mode, acc)
        else:
            with pytest.raises(ValueError):
                U.MulticlassAccuracy_fn(x, t, mode)
        assert isinstance(dice, np.ndarray if m == 0 else np.float64)
        assert isinstance(iou, np.ndarray if m == 0 else np.float64)


@pytest.mark.parametrize('key', ['c2', 'c3', 'c5', 'c8', 'c5one'])
def test_fixture_cpu(gold, key):
    check_fixture(gold, key, lambda x, t: (torch.from_numpy(x), torch.from_numpy(t)))


def test_fixture_numpy_and_target_dtypes(gold):
    check_fixture(gold, 'c5', lambda x, t: (x, t))
    check_fixture(gold, 'c3', lambda x, t: (torch.from_numpy(x), torch.from_numpy(t).float()))
    check_fixture(gold, 'c8', lambda x, t: (torch.from_numpy(x), torch.from_numpy(t).to(torch.uint8)))


@pytest.mark.parametrize('key', ['c2', 'c5', 'c8'])
def test_index_targets_equal_one_hot(gold, key):
    check_fixture(gold, key, lambda x, t: (torch.from_numpy(x), torch.from_numpy(t.argmax(axis=1))))
    from aide_amd.utils import multiclass_counts
    x, t = gold[key + '/logits'], gold[key + '/onehot']
    assert np.array_equal(multiclass_counts(x, t), multiclass_counts(x, t.argmax(axis=1)))


@pytest.mark.parametrize('c', [2, 3, 4, 6, 7, 8])
def test_accuracy_needs_five_classes(c):
    from aide_amd.utils import MulticlassAccuracy_fn
    x = torch.zeros(2, c, 4, 4)
    with pytest.raises(ValueError, match='5 classes'):
        MulticlassAccuracy_fn(x, torch.zeros(2, c, 4, 4))
    with pytest.raises(ValueError, match='5 classes'):
        MulticlassAccuracy_fn(x, torch.zeros(2, 4, 4, dtype=torch.int64), mode='train3_multidomainl_normalcl')


def test_counts_rules_host():
    """ties -> lowest class, the first NaN wins, an index outside [0, C) belongs to no class but its pixel is predicted"""
    from aide_amd.utils import multiclass_counts
    x = np.zeros((1, 3, 1, 4), np.float32)
    x[0, :, 0, 1] = [0.0, np.nan, np.nan]
    x[0, :, 0, 2] = [1.0, 5.0, np.nan]
    x[0, :, 0, 3] = [0.0, 2.0, 2.0]
    t = np.array([[[0, 1, 2, 255]]], np.int64)
    cnt = multiclass_counts(x, t)                 # predictions 0, 1, 2, 1
    assert cnt.dtype == np.int64 and cnt.tolist() == [[[1, 1, 1], [1, 2, 1], [1, 1, 1]]]


def test_argument_errors_host():
    from aide_amd.utils import MulticlassDice_fn
    for x, t in ((torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)), (torch.zeros(1, 9, 4, 4), torch.zeros(1, 9, 4, 4)),
                 (torch.zeros(1, 3, 4, 4, dtype=torch.float16), torch.zeros(1, 3, 4, 4)),
                 (torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 5)), (torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4))):
        with pytest.raises(RuntimeError):
            MulticlassDice_fn(x, t)


def host_loop(logits, index, hw):
    """the reference's loops over a list of images, written out on the counts: -> dict like MulticlassMeter.compute()"""
    c = logits.shape[1]
    pred = torch.argmax(torch.from_numpy(logits), dim=1).numpy()
    dice, iou, tp, si, st = np.zeros(c), np.zeros(c), np.zeros(c), np.zeros(c), np.zeros(c)
    for p, t in zip(pred, index):
        for k in range(c):
            a, b, d = int(((p == k) & (t == k)).sum()), int((p == k).sum()), int((t == k).sum())
            dice[k] += 1.0 if b + d == 0 else np.float64(2 * a) / np.float64(b + d)
            iou[k] += 1.0 if b + d == 0 else np.float64(a) / np.float64(b + d - a)
            tp[k] += a
            si[k] += b
            st[k] += d
    n = float(len(pred))
    return dict(dice=dice / n, iou=iou / n, TP=tp / n, TN=(n * hw - si - st + tp) / n, FP=(si - tp) / n, FN=(st - tp) / n,
                images=len(pred))


def test_meter_host():
    from aide_amd.utils import MulticlassMeter, MulticlassDice_fn
    rng = np.random.RandomState(3)
    c, h, w = 5, 6, 10
    x = rng.randn(6, c, h, w).astype(np.float32)
    x[:, 4] = -9.0
    t = rng.randint(0, 4, size=(6, h, w))
    t[2] = 0
    meter = MulticlassMeter(c, 'cpu')
    for a, b in ((0, 1), (1, 4), (4, 6)):
        assert meter.update(torch.from_numpy(x[a:b]), torch.from_numpy(t[a:b])) is None
    got, want = meter.compute(), host_loop(x, t, h * w)
    assert got['images'] == 6
    for k in ('dice', 'iou') + CONF:
        assert same_bits(got[k], want[k]), (k, got[k], want[k])
    assert same_bits(got['dice'], MulticlassDice_fn(x, t))
    meter.reset()
    meter.update(x[:1], t[:1])
    assert meter.compute()['images'] == 1 and same_bits(meter.compute()['dice'], MulticlassDice_fn(x[:1], t[:1]))


def class_sums(p, t, c):
    """per-class sums of two label volumes, stated directly"""
    n = p.size
    out = dict((k, []) for k in ('Dice', 'IoU') + CONF)
    for k in range(c):
        i, j = (p == k).astype(np.int64), (t == k).astype(np.int64)
        tp, si, st = int((i * j).sum()), int(i.sum()), int(j.sum())
        with np.errstate(divide='ignore', invalid='ignore'):
            out['Dice'].append(np.float64(2 * tp) / np.float64(si + st))
            out['IoU'].append(np.float64(tp) / np.float64(si + st - tp))
        out['TP'].append(tp)
        out['TN'].append(n - si - st + tp)
        out['FP'].append(si - tp)
        out['FN'].append(st - tp)
    return dict((k, np.asarray(v)) for k, v in out.items())


@pytest.mark.parametrize('c', [2, 5, 8])
def test_case_scores_per_class_numpy(c):
    from aide_amd.inference import case_scores
    rng = np.random.RandomState(c)
    p = rng.randint(0, c + 2, size=(7, 9, 3)).astype(np.int64)      # labels >= C present in the prediction
    t = rng.randint(0, c, size=(7, 9, 3)).astype(np.uint8)
    if c > 2:
        p[p == c - 1] = 0
        t[t == c - 1] = 0                                           # a class in neither volume: 0 / 0 -> nan
    got, want = case_scores(p, t, num_classes=c), class_sums(p, t, c)
    for k in want:
        assert same_bits(got[k], want[k]), (k, got[k], want[k])
    got = case_scores(torch.from_numpy(p), torch.from_numpy(t), num_classes=c)
    for k in want:
        assert same_bits(got[k], want[k]), (k, got[k], want[k])
    with pytest.raises(RuntimeError):
        case_scores(p, t, num_classes=9)


def test_case_scores_default_unchanged():
    from aide_amd.inference import case_scores
    rng = np.random.RandomState(1)
    p = (rng.rand(16, 16, 5) > 0.6).astype(np.int64)
    t = (rng.rand(16, 16, 5) > 0.5).astype(np.int64)
    spt, sp, st, n = int((p * t).sum()), int(p.sum()), int(t.sum()), p.size
    want = dict(Dice=np.float64(2 * spt) / np.float64(sp + st), IoU=np.float64(spt) / np.float64(sp + st - spt), TP=spt,
                TN=n - sp - st + spt, FP=sp - spt, FN=st - spt)
    for got in (case_scores(p, t), case_scores(p, t, num_classes=None), case_scores(p, t, None)):
        assert sorted(got) == sorted(want)
        for k in want:
            assert type(got[k]) is type(want[k]) and got[k] == want[k], (k, got[k], want[k])
