"""Host side of the per-case evaluation (include/aide_hip.h "per-case evaluation", aide_amd/inference.py): the new entry
points are declared and exported, the CPU scores follow the reference's formulas, CPU inputs keep the CPU path, and the
device wrappers reject bad arguments before anything is launched."""
import subprocess

import numpy as np
import pytest
import torch

NEW = ('aide_lcc3d_ws_bytes', 'aide_keep_largest_cc3d', 'aide_case_confusion')


@pytest.fixture(scope='module')
def built():
    from aide_amd.build import build
    return build(verbose=False)


def test_eval_entry_points_declared_and_exported(built):
    from aide_amd._lib import lib, parse_header
    protos = parse_header()
    out = subprocess.run(['nm', '-D', '--defined-only', built], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW:
        assert name in protos and name in exported, name
    assert len(protos['aide_keep_largest_cc3d'][1]) == 10 and len(protos['aide_case_confusion'][1]) == 15


def test_eval_entry_points_reject_without_launch(built):
    """Size limits of the C ABI: answered on the host, before any HIP call."""
    from aide_amd._lib import lib
    assert lib.aide_lcc3d_ws_bytes(2 ** 31) == 0
    assert lib.aide_lcc3d_ws_bytes(-1) == 0
    assert lib.aide_lcc3d_ws_bytes(1000) >= 8 * 1000 + 16
    assert lib.aide_keep_largest_cc3d(None, 2 ** 16, 2 ** 15, 1, 2 ** 15, 1, 1, None, None, None) < 0     # 2^31 voxels
    assert lib.aide_keep_largest_cc3d(None, -1, 4, 4, 16, 4, 1, None, None, None) < 0
    assert lib.aide_case_confusion(None, 0, 1, 1, 1, None, 0, 1, 1, 1, 2 ** 16, 2 ** 15, 1, None, None) < 0
    assert lib.aide_case_confusion(None, 2, 1, 1, 1, None, 0, 1, 1, 1, 1, 1, 1, None, None) < 0


def _reference_scores(p, t):
    """evalchaos_comparison_1cases.py:116-141 restated with int64 arithmetic."""
    i, f = p.reshape(-1).astype(np.int64), t.reshape(-1).astype(np.int64)
    with np.errstate(divide='ignore', invalid='ignore'):
        dice = 2 * np.sum(i * f) / (np.sum(i) + np.sum(f))
        iou = np.sum(i * f) / (np.sum(i) + np.sum(f) - np.sum(i * f))
    return dict(Dice=dice, IoU=iou, TP=np.sum(i * f), TN=np.sum((1 - i) * (1 - f)), FP=np.sum(i * (1 - f)),
                FN=np.sum((1 - i) * f))


def _same(a, b):
    assert set(a) == set(b)
    for k in ('TP', 'TN', 'FP', 'FN'):
        assert int(a[k]) == int(b[k]), (k, a[k], b[k])
    for k in ('Dice', 'IoU'):
        x, y = np.float64(a[k]), np.float64(b[k])
        assert (np.isnan(x) and np.isnan(y)) or x == y, (k, x, y)


def test_case_scores_numpy_matches_reference_formulas():
    from aide_amd.inference import case_scores
    rng = np.random.RandomState(3)
    cases = [
        ((rng.rand(9, 11, 5) < 0.3).astype(np.uint8), (rng.rand(9, 11, 5) < 0.4).astype(np.int64)),
        (rng.randint(0, 3, (6, 7, 4)).astype(np.int64), rng.randint(0, 4, (6, 7, 4)).astype(np.int64)),  # non-binary
        (np.zeros((5, 5, 3), np.uint8), (rng.rand(5, 5, 3) < 0.5).astype(np.int64)),                     # empty prediction
        (np.zeros((4, 4, 2), np.int64), np.zeros((4, 4, 2), np.int64)),                                 # 0/0 -> nan
        (rng.randint(-2, 3, (3, 8, 8)).astype(np.int64), rng.randint(-1, 2, (3, 8, 8)).astype(np.int64)),
    ]
    for p, t in cases:
        got = case_scores(p, t)
        _same(got, _reference_scores(p, t))
    # x/0 -> inf, as numpy's true division
    p = np.array([1, -1], np.int64)
    t = np.array([1, -1], np.int64)                                     # sum p + sum t = 0, TP = 2
    s = case_scores(p, t)
    assert s['Dice'] == np.inf and s['IoU'] == -1.0
    p, t = np.array([2, 0], np.int64), np.array([1, -1], np.int64)     # sum p + sum t - TP = 2 + 0 - 2 = 0
    s = case_scores(p, t)
    assert s['IoU'] == np.inf and s['Dice'] == 2.0 * 2 / 2


def test_cpu_inputs_keep_cpu_path():
    """numpy arrays and CPU torch tensors go through the unchanged CPU code."""
    from aide_amd.inference import keep_largest_connected_components as keep, case_scores
    rng = np.random.RandomState(7)
    m = rng.randint(0, 3, (6, 9, 4)).astype(np.int64)
    ref = keep(m)
    got = keep(torch.from_numpy(m))
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, ref)
    p = (rng.rand(5, 6, 7) < 0.5).astype(np.int64)
    t = (rng.rand(5, 6, 7) < 0.5).astype(np.int64)
    _same(case_scores(torch.from_numpy(p), torch.from_numpy(t)), case_scores(p, t))


def test_device_wrappers_reject_bad_arguments():
    """The checks of the device path run before anything is launched (meta tensors: no memory, no device)."""
    from aide_amd.inference import _lcc_args, _confusion_args
    _lcc_args(torch.zeros(2, 3, 4, dtype=torch.int64))
    _lcc_args(torch.zeros(2, 3, 4, dtype=torch.uint8))
    for bad in (torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, 4, 5, dtype=torch.int64),
                torch.zeros(2, 3, 4, dtype=torch.float32), torch.empty(2 ** 16, 2 ** 15, 1, dtype=torch.int64, device='meta')):
        with pytest.raises(RuntimeError):
            _lcc_args(bad)
    _lcc_args(torch.empty(2 ** 16, 2 ** 15 - 1, 1, dtype=torch.int64, device='meta'))     # 2^31 - 2^16 voxels: fine
    a = torch.zeros(4, 5, 6, dtype=torch.int64)
    _confusion_args(a, a.to(torch.uint8))
    with pytest.raises(RuntimeError):
        _confusion_args(a, torch.zeros(4, 6, 5, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        _confusion_args(a, a.float())
    with pytest.raises(RuntimeError):
        _confusion_args(torch.zeros((), dtype=torch.int64), torch.zeros((), dtype=torch.int64))
    big = torch.empty(2 ** 31, dtype=torch.uint8, device='meta')
    with pytest.raises(RuntimeError):
        _confusion_args(big, big)
