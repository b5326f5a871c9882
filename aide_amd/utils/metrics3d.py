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
Percentiles (HD95) and the surface Dice at a tolerance (NSD).  A = the multiset {D_T(v) : v in border(P)} (n_P values),
B = {D_P(v) : v in border(T)} (n_T values), A+B their multiset union.
  percentile q (0 <= q <= 100) of a multiset of m >= 1 values x[0] <= ... <= x[m-1]:
               pos = (m - 1) * q / 100.0, evaluated left to right in IEEE float64; lo = floor(pos); hi = min(lo + 1, m - 1);
               value = x[lo] + (x[hi] - x[lo]) * (pos - lo): numpy's 'linear' method up to the rounding of pos.  q = 0 is the
               minimum, q = 100 the maximum exactly ((m - 1) * 100 / 100 is exact)
  HD_pred[q]   percentile of A; HD_target[q] of B; HD[q] = max of the two (the max-of-directed convention, MONAI's);
               HD_pooled[q] = percentile of A+B (medpy's hd95); all NaN when n_P == 0 or n_T == 0
  n_pred_within[tau] = |{a in A : a <= tau}| for a tolerance tau >= 0, n_target_within[tau] the same for B
  NSD[tau]     (n_pred_within + n_target_within) / (n_P + n_T) in float64, NaN when either border is empty: the voxel-count
               form of Nikolov et al.'s surface Dice
HIP tensors go through aide_surface3d_scores, or aide_surface3d_scores_select when percentiles or tolerances are asked for
(aide_amd/csrc/surface3d.hip); numpy arrays and CPU tensors through scipy and numpy, which is the definition above.
select_model() is the device's selection algorithm in numpy."""
import math

import numpy as np
import torch

from .._lib import lib, check
from ..ops import ptr, stream_ptr
from ..inference import Dice3d_fn, case_scores  # noqa: F401
from ..volumes import classes, device_pair, spacing as _spacing, u8, workspace


def IoU3d_fn(inputs, targets):
    """evalchaos_comparison_1cases.py:125-132: sum(i*t) / (sum i + sum t - sum(i*t)), float64."""
    return case_scores(inputs, targets)['IoU']


def TP_TN_FP_FN3d(inputs, targets):
    """evalchaos_comparison_1cases.py:134-141 -> (TP, TN, FP, FN)."""
    s = case_scores(inputs, targets)
    return s['TP'], s['TN'], s['FP'], s['FN']


def _classes(num_classes):
    if num_classes is None:
        return [-1]
    return list(range(1, classes(num_classes, 'surface_scores', strict=False)))


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


def _numbers(values, what, ok):
    """None -> (); 1 .. 4 numbers that pass `ok` -> tuple of floats; anything else: ValueError"""
    if values is None:
        return ()
    try:
        v = tuple(float(x) for x in values)
    except (TypeError, ValueError):
        raise ValueError('%s: 1 .. 4 numbers expected, got %r' % (what, values))
    if not 1 <= len(v) <= 4 or not all(math.isfinite(x) and ok(x) for x in v):
        raise ValueError('%s: 1 .. 4 finite numbers in range expected, got %r' % (what, values))
    return v


def percentile_rank(m, q):
    """-> pos, lo, hi of percentile q in a multiset of m >= 1 values (the definition in the module docstring)"""
    pos = (m - 1) * float(q) / 100.0
    lo = int(math.floor(pos))
    return pos, lo, min(lo + 1, m - 1)


def select_model(keys_uint64, ranks):
    """The order statistics `ranks` (0-based) of the uint64 keys, by the digit walk of the device (sel_hist / sel_choose in
    aide_amd/csrc/surface3d.hip): eight passes from the most significant byte down; per pass a histogram of the byte over the
    keys that carry the prefix chosen so far, the first bin whose running count exceeds the rank, rank -= the count before it.
    Equal keys share every digit, so a run of ties is one bin.  -> uint64 [len(ranks)]"""
    keys = np.ascontiguousarray(keys_uint64, dtype=np.uint64).reshape(-1)
    res = np.zeros(len(ranks), np.uint64)
    for k, rank in enumerate(ranks):
        rank = int(rank)
        if not 0 <= rank < keys.size:
            raise ValueError('select_model: rank %d outside [0, %d)' % (rank, keys.size))
        live, prefix = keys, 0
        for p in range(8):
            shift = np.uint64(56 - 8 * p)
            digit = ((live >> shift) & np.uint64(255)).astype(np.int64)
            incl = np.cumsum(np.bincount(digit, minlength=256))
            d = int(np.searchsorted(incl, rank, side='right'))          # the first bin with excl <= rank < incl
            rank -= int(incl[d - 1]) if d else 0
            prefix = (prefix << 8) | d
            live = live[digit == d]
        res[k] = prefix
    return res


def _select_host(maps, n_p, n_t, qs, taus):
    """-> within int64 [4,2], lo int64 [3,4], x_lo, x_hi float64 [3,4] in the layout of aide_surface3d_scores_select's words,
    from the two distance maps: np.sort is the order statistic"""
    within, lo = np.zeros((4, 2), np.int64), np.zeros((3, 4), np.int64)
    x_lo, x_hi = np.zeros((3, 4), np.float64), np.zeros((3, 4), np.float64)
    if n_p and n_t:
        a, b = (np.sort(m[m >= 0]) for m in maps)
        sets = (a, b, np.sort(np.concatenate([a, b])))
        for j, tau in enumerate(taus):
            within[j] = np.count_nonzero(a <= tau), np.count_nonzero(b <= tau)
        for s, x in enumerate(sets):
            for j, q in enumerate(qs):
                _, lo[s, j], hi = percentile_rank(x.size, q)
                x_lo[s, j], x_hi[s, j] = x[lo[s, j]], x[hi]
    return within, lo, x_lo, x_hi


def _raw_device(pred, target, sp, cls_values, distances, qs=(), taus=()):
    """-> int64 [K,4], float64 [K,4] (numpy) and the distance tensor [K,2,d0,d1,d2] or None, for the K entries of `cls_values`:
    K calls enqueued back to back on one workspace, one copy of K * 8 words.  With percentiles or tolerances the calls are
    aide_surface3d_scores_select's, the copy is K * 52 words, and a fourth value carries (within [K,4,2], lo [K,3,4], x_lo,
    x_hi [K,3,4]); None otherwise."""
    p, t = device_pair(pred, target, 'surface_scores')
    k, n = len(cls_values), p.numel()
    select = bool(qs or taus)
    out = torch.zeros(k, 52 if select else 8, device=p.device, dtype=torch.int64)
    dist = torch.full((k, 2) + tuple(p.shape), -1.0, device=p.device, dtype=torch.float64) if distances else None
    if n and select:
        import ctypes
        cq, ct = (ctypes.c_double * 4)(*qs), (ctypes.c_double * 4)(*taus)
        ws = workspace(lib.aide_surface3d_select_ws_bytes, p)
        for i, c in enumerate(cls_values):
            check(lib.aide_surface3d_scores_select(ptr(p), u8(p), *p.stride(), ptr(t), u8(t), *t.stride(), *p.shape, *sp, c, cq,
                                                   len(qs), ct, len(taus), ptr(out[i]), ptr(dist[i]) if distances else None,
                                                   ptr(ws), stream_ptr()), 'surface3d_scores_select')
    elif n:
        ws = workspace(lib.aide_surface3d_ws_bytes, p)
        for i, c in enumerate(cls_values):
            check(lib.aide_surface3d_scores(ptr(p), u8(p), *p.stride(), ptr(t), u8(t), *t.stride(), *p.shape, *sp, c, ptr(out[i]),
                                            ptr(dist[i]) if distances else None, ptr(ws), stream_ptr()), 'surface3d_scores')
    words = out.cpu().numpy()
    sel = None
    if select:
        tri = words[:, 16:52].reshape(k, 3, 4, 3)
        sel = (words[:, 8:16].reshape(k, 4, 2).copy(), tri[..., 0].copy(), tri[..., 1].copy().view(np.float64),
               tri[..., 2].copy().view(np.float64))
    return words[:, :4].copy(), words[:, 4:8].copy().view(np.float64), dist, sel


def _scores(ints, flts):
    """raw words [K,4] + [K,4] -> RAVD, ASSD, MSSD float64 [K]"""
    n_p, n_t, v_p, v_t = (ints[:, j] for j in range(4))
    with np.errstate(divide='ignore', invalid='ignore'):
        ravd = np.abs(v_p - v_t).astype(np.float64) / v_t.astype(np.float64) * 100.0
        assd = (flts[:, 0] + flts[:, 1]) / (n_p + n_t).astype(np.float64)
    mssd = np.maximum(flts[:, 2], flts[:, 3])
    empty = (n_p == 0) | (n_t == 0)
    return ravd, np.where(empty, np.nan, assd), np.where(empty, np.nan, mssd)


def _select_scores(ints, sel, qs, taus):
    """the words of the selection -> dict of the percentile and tolerance entries, arrays [K, Q] / [K, T]"""
    within, lo, x_lo, x_hi = sel
    n_p, n_t = ints[:, 0], ints[:, 1]
    empty = (n_p == 0) | (n_t == 0)
    res = {}
    if qs:
        hd = np.full((3, len(ints), len(qs)), np.nan, np.float64)
        for k in np.flatnonzero(~empty):
            for s, m in enumerate((int(n_p[k]), int(n_t[k]), int(n_p[k] + n_t[k]))):
                for j, q in enumerate(qs):
                    pos = percentile_rank(m, q)[0]
                    a, b = x_lo[k, s, j], x_hi[k, s, j]
                    hd[s, k, j] = a + (b - a) * (pos - float(lo[k, s, j]))
        res.update(percentiles=np.array(qs, np.float64), HD=np.maximum(hd[0], hd[1]), HD_pred=hd[0], HD_target=hd[1],
                   HD_pooled=hd[2])
    if taus:
        w = np.where(empty[:, None, None], 0, within[:, :len(taus)])
        with np.errstate(divide='ignore', invalid='ignore'):
            nsd = (w[:, :, 0] + w[:, :, 1]).astype(np.float64) / (n_p + n_t).astype(np.float64)[:, None]
        res.update(tolerances=np.array(taus, np.float64), NSD=np.where(empty[:, None], np.nan, nsd),
                   n_pred_within=w[:, :, 0].copy(), n_target_within=w[:, :, 1].copy())
    return res


_PER_CASE = ('percentiles', 'tolerances')          # entries of _select_scores that carry no class axis


def surface_scores(pred, target, spacing, num_classes=None, distances=False, percentiles=None, tolerances=None):
    """dict(RAVD, ASSD, MSSD, n_pred, n_target, V_pred, V_target) of a predicted label volume against its target, both of the
    logical shape (d0, d1, d2), with `spacing` = the edge lengths of a voxel along those dims (for the reference's [H,W,S]
    volumes the evaluation script's `voxelspacing`).  num_classes=C (2 .. 8): every entry an array [C] (scores float64 with
    NaN for the background entry 0, counts int64 with 0 there); a label outside [0, C) belongs to no class.  distances=True
    adds dist_pred (D_T at the border voxels of the prediction) and dist_target (D_P at those of the target), float64 shaped
    like the volume ([C, ...] with classes), -1.0 everywhere else: `torch.quantile` of the non-negative entries gives any
    percentile, at the cost of a host synchronisation; `percentiles` does it on the device.
    percentiles=(q, ...), tolerances=(tau, ...), None or 1 .. 4 numbers each (0 <= q <= 100, tau >= 0; ValueError otherwise),
    add, and only then: percentiles, HD, HD_pred, HD_target, HD_pooled (float64 [Q]; [C, Q] with classes, row 0 NaN) and
    tolerances, NSD (float64 [T] or [C, T]), n_pred_within, n_target_within (int64, row 0 zeros), as defined in the module
    docstring: HD of percentiles=(95,) is HD95.  HIP tensors then take aide_surface3d_scores_select: 21 launches per class
    whatever Q and T are, still one copy ([C][52] words) and no other host read.
    HIP tensors (integer dtypes, any strides: a [S,H,W] tensor passed as .permute(1, 2, 0) works): five launches per class,
    enqueued back to back, one copy of [C][8] words, the divisions on the host in float64; the distance maps stay on the device.
    numpy arrays and CPU tensors: scipy (binary_erosion, distance_transform_edt), numpy maps."""
    sp = _spacing(spacing, 'surface_scores')
    cls_values = _classes(num_classes)
    qs = _numbers(percentiles, 'percentiles', lambda v: 0.0 <= v <= 100.0)
    taus = _numbers(tolerances, 'tolerances', lambda v: v >= 0.0)
    select = bool(qs or taus)
    dev = [x for x in (pred, target) if isinstance(x, torch.Tensor) and x.is_cuda]
    if dev:
        pred = torch.as_tensor(pred, device=dev[0].device)
        target = torch.as_tensor(target, device=dev[0].device)
        if pred.dim() != 3:
            raise RuntimeError('surface_scores: 3-D volumes expected, got %d dims' % pred.dim())
        ints, flts, dist, sel = _raw_device(pred, target, sp, cls_values, distances, qs, taus)
        maps = (dist[:, 0], dist[:, 1]) if distances else None
    else:
        p, t = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (pred, target))
        if p.shape != t.shape:
            raise RuntimeError('surface_scores: shape mismatch %s vs %s' % (p.shape, t.shape))
        if p.ndim != 3:
            raise RuntimeError('surface_scores: 3-D volumes expected, got %d dims' % p.ndim)
        raw = [_raw_host(p, t, sp, c, distances or select) for c in cls_values]
        ints = np.array([r[0] for r in raw], np.int64).reshape(-1, 4)
        flts = np.array([r[1] for r in raw], np.float64).reshape(-1, 4)
        maps = tuple(np.stack([r[2][k] for r in raw]) for k in range(2)) if distances else None
        if select:
            sel = tuple(np.stack(x) for x in zip(*(_select_host(r[2], r[0][0], r[0][1], qs, taus) for r in raw)))
    ravd, assd, mssd = _scores(ints, flts)
    extra = _select_scores(ints, sel, qs, taus) if select else {}
    if num_classes is None:
        res = dict(RAVD=ravd[0], ASSD=assd[0], MSSD=mssd[0], n_pred=int(ints[0, 0]), n_target=int(ints[0, 1]),
                   V_pred=int(ints[0, 2]), V_target=int(ints[0, 3]))
        if distances:
            res.update(dist_pred=maps[0][0], dist_target=maps[1][0])
        res.update((k, v if k in _PER_CASE else v[0]) for k, v in extra.items())
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
    for key, v in extra.items():
        res[key] = v if key in _PER_CASE else np.concatenate([np.full_like(v[:1], 0 if v.dtype == np.int64 else np.nan), v])
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


def HD95_fn(pred, target, spacing=(1.0, 1.0, 1.0), pooled=False):
    """95th percentile Hausdorff distance in the unit of `spacing`: the larger of the two directed percentiles (MONAI's
    convention), or with pooled=True the percentile of the two sets of distances taken together (medpy's hd95)"""
    return surface_scores(pred, target, spacing, percentiles=(95.0,))['HD_pooled' if pooled else 'HD'][0]


def NSD3d_fn(pred, target, tolerance, spacing=(1.0, 1.0, 1.0)):
    """normalised surface Dice: the share of the border voxels of both volumes that lie within `tolerance` (in the unit of
    `spacing`, <=) of the other volume's border"""
    return surface_scores(pred, target, spacing, tolerances=(tolerance,))['NSD'][0]
