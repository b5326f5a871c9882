"""Per-case 3-D metrics under the reference's module name (its utils/metrics3d.py is four import lines): the evaluation
script's Dice3d_fn / IoU3d_fn / TP_TN_FP_FN3d (evalchaos_comparison_1cases.py:116-141) and the three scores of the CHAOS
challenge that need the voxel spacing the script reads (`voxelspacing`, :181, 192-194) and never uses: RAVD, ASSD, MSSD.

Definitions, for a prediction P and a target T of logical shape (d0, d1, d2) and spacing (sp0, sp1, sp2):
  foreground   X != 0, or X == c for class c when num_classes is given
  border       foreground with at least one of the six face neighbours not foreground or outside the volume
               (fg & ~binary_erosion(fg, generate_binary_structure(3, 1), border_value=0))
  D_X(v)       min over u in border(X) of sqrt(sum_k (sp_k * (v_k - u_k))^2), float64, exact Euclidean
  n_P, n_T     border voxel counts; V_P, V_T foreground voxel counts
  S_PT, M_PT   sum and max of D_T over border(P); S_TP, M_TP the other direction
  ASSD         (S_PT + S_TP) / (n_P + n_T); MSSD = max(M_PT, M_TP); both NaN when n_P == 0 or n_T == 0
  RAVD         float64(|V_P - V_T|) / float64(V_T) * 100.0, numpy's true division (x/0 -> inf, 0/0 -> nan)
HIP tensors go through aide_surface3d_scores (aide_amd/csrc/surface3d.hip); numpy arrays and CPU tensors through scipy, which
is the definition above."""
import math

import numpy as np
import torch

from .._lib import lib, check
from ..ops import ptr, stream_ptr
from ..inference import Dice3d_fn, case_scores, _confusion_args, _as3d  # noqa: F401


def IoU3d_fn(inputs, targets):
    """evalchaos_comparison_1cases.py:125-132: sum(i*t) / (sum i + sum t - sum(i*t)), float64."""
    return case_scores(inputs, targets)['IoU']


def TP_TN_FP_FN3d(inputs, targets):
    """evalchaos_comparison_1cases.py:134-141 -> (TP, TN, FP, FN)."""
    s = case_scores(inputs, targets)
    return s['TP'], s['TN'], s['FP'], s['FN']


def _spacing(spacing):
    try:
        sp = tuple(float(v) for v in spacing)
    except TypeError:
        raise ValueError('spacing: three positive numbers expected, got %r' % (spacing,))
    if len(sp) != 3 or not all(math.isfinite(v) and v > 0.0 for v in sp):
        raise ValueError('spacing: three positive finite numbers expected, got %r' % (spacing,))
    return sp


def _classes(num_classes):
    if num_classes is None:
        return [-1]
    c = int(num_classes)
    if not 2 <= c <= 8:
        raise RuntimeError('surface_scores: num_classes %d, 2 .. 8 are supported' % c)
    return list(range(1, c))


def _raw_host(p, t, sp, cls, distances):
    """-> (n_P, n_T, V_P, V_T), (S_PT, S_TP, M_PT, M_TP), (dist_P, dist_T) or None: the scipy statement of the definitions"""
    from scipy import ndimage
    fg = [(x != 0) if cls < 0 else (x == cls) for x in (p, t)]
    st = ndimage.generate_binary_structure(3, 1)
    bd = [f & ~ndimage.binary_erosion(f, st, border_value=0) if f.size else f for f in fg]
    n = [int(b.sum()) for b in bd]
    maps = [np.full(p.shape, -1.0, np.float64) for _ in range(2)]
    s, m = [0.0, 0.0], [0.0, 0.0]
    if n[0] and n[1]:
        for k in range(2):                        # k = 0: the border of P measured against T
            d = ndimage.distance_transform_edt(~bd[1 - k], sampling=sp)[bd[k]]
            maps[k][bd[k]] = d
            s[k], m[k] = float(np.sum(d)), float(np.max(d))
    return (n[0], n[1], int(fg[0].sum()), int(fg[1].sum())), (s[0], s[1], m[0], m[1]), maps if distances else None


def _raw_device(pred, target, sp, classes, distances):
    """-> int64 [K,4], float64 [K,4] (numpy) and the distance tensor [K,2,d0,d1,d2] or None, for the K entries of `classes`:
    K calls enqueued back to back on one workspace, one copy of K * 8 words."""
    _confusion_args(pred, target)
    p, t = _as3d(pred), _as3d(target)
    k, n = len(classes), p.numel()
    out = torch.zeros(k, 8, device=p.device, dtype=torch.int64)
    dist = torch.full((k, 2) + tuple(p.shape), -1.0, device=p.device, dtype=torch.float64) if distances else None
    if n:
        ws = torch.empty(lib.aide_surface3d_ws_bytes(n), device=p.device, dtype=torch.uint8)
        for i, c in enumerate(classes):
            check(lib.aide_surface3d_scores(ptr(p), int(p.dtype == torch.uint8), *p.stride(), ptr(t), int(t.dtype == torch.uint8),
                                            *t.stride(), *p.shape, sp[0], sp[1], sp[2], c, ptr(out[i]),
                                            ptr(dist[i]) if distances else None, ptr(ws), stream_ptr()), 'surface3d_scores')
    words = out.cpu().numpy()
    return words[:, :4].copy(), words[:, 4:].copy().view(np.float64), dist


def _scores(ints, flts):
    """raw words [K,4] + [K,4] -> RAVD, ASSD, MSSD float64 [K]"""
    n_p, n_t, v_p, v_t = (ints[:, j] for j in range(4))
    with np.errstate(divide='ignore', invalid='ignore'):
        ravd = np.abs(v_p - v_t).astype(np.float64) / v_t.astype(np.float64) * 100.0
        assd = (flts[:, 0] + flts[:, 1]) / (n_p + n_t).astype(np.float64)
    mssd = np.maximum(flts[:, 2], flts[:, 3])
    empty = (n_p == 0) | (n_t == 0)
    return ravd, np.where(empty, np.nan, assd), np.where(empty, np.nan, mssd)


def surface_scores(pred, target, spacing, num_classes=None, distances=False):
    """dict(RAVD, ASSD, MSSD, n_pred, n_target, V_pred, V_target) of a predicted label volume against its target, both of the
    logical shape (d0, d1, d2), with `spacing` = the edge lengths of a voxel along those dims (for the reference's [H,W,S]
    volumes the evaluation script's `voxelspacing`).  num_classes=C (2 .. 8): every entry an array [C] (scores float64 with
    NaN for the background entry 0, counts int64 with 0 there); a label outside [0, C) belongs to no class.  distances=True
    adds dist_pred (D_T at the border voxels of the prediction) and dist_target (D_P at those of the target), float64 shaped
    like the volume ([C, ...] with classes), -1.0 everywhere else: `torch.quantile` of the non-negative entries gives any
    percentile (HD95).
    HIP tensors (integer dtypes, any strides: a [S,H,W] tensor passed as .permute(1, 2, 0) works): five launches per class,
    enqueued back to back, one copy of [C][8] words, the divisions on the host in float64; the distance maps stay on the device.
    numpy arrays and CPU tensors: scipy (binary_erosion, distance_transform_edt), numpy maps."""
    sp = _spacing(spacing)
    classes = _classes(num_classes)
    dev = [x for x in (pred, target) if isinstance(x, torch.Tensor) and x.is_cuda]
    if dev:
        pred = torch.as_tensor(pred, device=dev[0].device)
        target = torch.as_tensor(target, device=dev[0].device)
        if pred.dim() != 3:
            raise RuntimeError('surface_scores: 3-D volumes expected, got %d dims' % pred.dim())
        ints, flts, dist = _raw_device(pred, target, sp, classes, distances)
        maps = (dist[:, 0], dist[:, 1]) if distances else None
    else:
        p, t = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (pred, target))
        if p.shape != t.shape:
            raise RuntimeError('surface_scores: shape mismatch %s vs %s' % (p.shape, t.shape))
        if p.ndim != 3:
            raise RuntimeError('surface_scores: 3-D volumes expected, got %d dims' % p.ndim)
        raw = [_raw_host(p, t, sp, c, distances) for c in classes]
        ints = np.array([r[0] for r in raw], np.int64).reshape(-1, 4)
        flts = np.array([r[1] for r in raw], np.float64).reshape(-1, 4)
        maps = tuple(np.stack([r[2][k] for r in raw]) for k in range(2)) if distances else None
    ravd, assd, mssd = _scores(ints, flts)
    if num_classes is None:
        res = dict(RAVD=ravd[0], ASSD=assd[0], MSSD=mssd[0], n_pred=int(ints[0, 0]), n_target=int(ints[0, 1]),
                   V_pred=int(ints[0, 2]), V_target=int(ints[0, 3]))
        if distances:
            res.update(dist_pred=maps[0][0], dist_target=maps[1][0])
        return res

    def with_background(a, fill):
        return np.concatenate([np.full(1, fill, a.dtype), a])
    res = dict(RAVD=with_background(ravd, np.nan), ASSD=with_background(assd, np.nan), MSSD=with_background(mssd, np.nan))
    for j, key in enumerate(('n_pred', 'n_target', 'V_pred', 'V_target')):
        res[key] = with_background(ints[:, j], 0)
    if distances:
        for key, m in zip(('dist_pred', 'dist_target'), maps):
            if isinstance(m, torch.Tensor):
                res[key] = torch.cat([torch.full_like(m[:1], -1.0), m])
            else:
                res[key] = np.concatenate([np.full_like(m[:1], -1.0), m])
    return res


def RAVD3d_fn(pred, target, spacing=(1.0, 1.0, 1.0)):
    """relative absolute volume difference in percent (does not depend on the spacing: every voxel has the same volume)"""
    return surface_scores(pred, target, spacing)['RAVD']


def ASSD3d_fn(pred, target, spacing=(1.0, 1.0, 1.0)):
    """average symmetric surface distance, in the unit of `spacing`"""
    return surface_scores(pred, target, spacing)['ASSD']


def MSSD3d_fn(pred, target, spacing=(1.0, 1.0, 1.0)):
    """maximum symmetric surface distance (the Hausdorff distance of the two borders), in the unit of `spacing`"""
    return surface_scores(pred, target, spacing)['MSSD']
