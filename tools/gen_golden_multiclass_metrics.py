"""Writes tests/golden/g25_multiclass_metrics.npz: the multi-class metrics as the reference computes them.

    python tools/gen_golden_multiclass_metrics.py

MulticlassDice_fn, MulticlassIoU_fn, MulticlassTP_TN_FP_FN, MulticlassAccuracy_fn and one_hot_result of the reference's
utils/metrics2d.py (:86-205) are taken out of the file's syntax tree and compiled IN MEMORY (oracle.gen_golden._ref_functions),
with `np.float = float` set in this process only: the functions use the alias that numpy 1.24 removed.  They are called in the
modes 'eval' and 'train3_multidomainl_normalcl' on the inputs below; inputs and results are stored, nothing of the reference's text.

Cases `c<C>`: C = 2, 3, 5, 8 with N = 3, H x W = 6 x 10 (HW = 60: no multiple of 64, of 8 or of the wave), and `c5one` with N = 1,
16 x 16.  MulticlassAccuracy_fn is recorded for C = 5 only: it raises ValueError for every other class count (asserted here).
Every case holds
  image 0, pixel (0, 0)   all C logits equal                         -> class 0
  image 0, pixel (0, 1)   classes 1 .. C-1 tie above class 0          -> class 1
  image 1 (N = 3)         the target is all background and the prediction uses classes 0 and 1 only (C = 2: class 0 only), so
                          the union is 0 for the classes above
  class C-1 (C >= 3)      never predicted and never present
Targets are the loaders' one-hot int64 [N,C,H,W]."""
import os
import sys
import warnings

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF, _ref_functions  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'g25_multiclass_metrics.npz')
METRICS = os.path.join(REF, 'utils', 'metrics2d.py')
MODES = ('eval', 'train3_multidomainl_normalcl')
NAMES = ['MulticlassDice_fn', 'MulticlassIoU_fn', 'MulticlassTP_TN_FP_FN', 'MulticlassAccuracy_fn', 'one_hot_result']


def make_case(c, n, h, w, seed):
    rng = np.random.RandomState(seed)
    logits = rng.randn(n, c, h, w).astype(np.float32)
    index = rng.randint(0, c, size=(n, h, w))
    if c >= 3:                                     # the last class: never predicted, never present
        logits[:, c - 1] = -10.0
        index[index == c - 1] = 0
    logits[0, :, 0, 0] = 0.25
    logits[0, 0, 0, 1] = -1.0
    logits[0, 1:, 0, 1] = 0.5
    if n > 1:
        index[1] = 0
        logits[1, 0] = 4.0
        logits[1, 1:] = -4.0
        if c >= 3:
            logits[1, 1, 2, 3:7] = 6.0
            logits[1, c - 1] = -10.0
    onehot = (index[:, None] == np.arange(c)[None, :, None, None]).astype(np.int64)
    return logits, onehot


def main():
    np.float = float                               # this process only: the alias the reference's functions use
    dice_fn, iou_fn, conf_fn, acc_fn, _ = _ref_functions(METRICS, NAMES, dict(np=np, torch=torch))
    out, cases = {}, []
    for key, c, n, h, w in (('c2', 2, 3, 6, 10), ('c3', 3, 3, 6, 10), ('c5', 5, 3, 6, 10), ('c8', 8, 3, 6, 10),
                            ('c5one', 5, 1, 16, 16)):
        logits, onehot = make_case(c, n, h, w, seed=100 + 7 * c + n)
        x, t = torch.from_numpy(logits), torch.from_numpy(onehot)
        pred = torch.argmax(x, dim=1).numpy()
        assert pred[0, 0, 0] == 0 and pred[0, 0, 1] == 1
        if c >= 3:
            assert not (pred == c - 1).any() and onehot[:, c - 1].sum() == 0
        if n > 1:
            assert onehot[1, 0].all() and set(np.unique(pred[1])) == ({0, 1} if c >= 3 else {0})
        out[key + '/logits'] = logits
        out[key + '/onehot'] = onehot
        for m, mode in enumerate(MODES):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)        # the reference's 0 / 0
                out['%s/m%d/dice' % (key, m)] = np.asarray(dice_fn(x.clone(), t.clone(), mode))
                out['%s/m%d/iou' % (key, m)] = np.asarray(iou_fn(x.clone(), t.clone(), mode))
                for name, v in zip(('TP', 'TN', 'FP', 'FN'), conf_fn(x.clone(), t.clone(), mode)):
                    out['%s/m%d/%s' % (key, m, name)] = np.asarray(v)
                if c == 5:
                    out['%s/m%d/accuracy' % (key, m)] = np.asarray(acc_fn(x.clone(), t.clone(), mode))
                else:
                    try:
                        acc_fn(x.clone(), t.clone(), mode)
                    except ValueError:
                        pass
                    else:
                        raise AssertionError('MulticlassAccuracy_fn did not raise for C = %d' % c)
            for name in ('dice', 'iou', 'TP', 'TN', 'FP', 'FN'):
                assert out['%s/m%d/%s' % (key, m, name)].dtype == np.float64
        assert out[key + '/m0/dice'].shape == (c,) and out[key + '/m1/dice'].shape == ()
        if n > 1 and c >= 3:                                           # unions of 0 gave 1.0 for several classes
            assert (out[key + '/m0/dice'][2:] >= 1.0 / n).all()
        cases.append(key)
    out['cases'] = np.asarray(cases)
    out['modes'] = np.asarray(MODES)
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))
    for key in cases:
        print(key, 'dice', out[key + '/m0/dice'], 'special', float(out[key + '/m1/dice']))


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
