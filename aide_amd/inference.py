"""Per-case inference of the training scripts, on device and batched.

Reference (train_files/trainchaos_comparison_1case.py:233-273, :275-314; the same loop in
trainchaos_proposed_30cases1labeled.py:373-493 and evalchaos_comparison_1cases.py:143-243): for every
slice of a case, bs=1: `argmax(softmax(net(inphase, outphase), dim=1), dim=1)` under `net.eval()` +
`no_grad`, `.cpu().numpy()` per slice, `np.stack(..., axis=-1)`, then skimage's largest connected
component and `Dice3d_fn` (the evaluation script: Dice, IoU, TP, TN, FP, FN).

Here the slices of a case go through the eval-mode kernels in batches (eval BatchNorm uses the running
statistics, so slices are independent and batching changes nothing but the launch count), the label
map is one kernel (`aide_label_map`), the largest-component filter and the confusion sums are kernels
too (`aide_keep_largest_cc3d`, `aide_case_confusion`), and only what the caller asks for leaves the device.
"""
import numpy as np
import torch

from ._lib import lib, check
from .ops import ptr, stream_ptr
from .ensemble import (VIEW_SETS, view_codes, view_apply_host, view_invert_host, view_stack, ensemble_vote,  # noqa: F401
                       ensemble_vote_host, ensemble_logits, predict_ensemble)
from .window import (window_grid, window_weights, window_stack, window_blend, window_blend_host,  # noqa: F401
                     predict_windows)
from .morphology import ball, erode, dilate, open_, close, distance_transform  # noqa: F401
from .resample import axis_table, resampled_shape, resample_image, resample_labels, resample_probs  # noqa: F401
from .postprocess import (MAX_TOP_K, MAX_BLOBS, PROPS_COLUMNS, LESION_COLUMNS, keep_largest_connected_components,  # noqa: F401
                          keep_largest_per_class, keep_components, fill_holes, label_components, region_table, lesion_counts,
                          lesion_scores, keep_largest_batched, _overlap, _starts)
from .volumes import classes, device_pair, spacing as _spacing, u8, volume_args


def label_map(logits):
    """[N,C,H,W] fp32 logits (C = 2 .. 8) -> [N,H,W] int64 labels = torch.argmax(F.softmax(logits, 1), 1)."""
    if logits.dim() != 4 or not 2 <= logits.shape[1] <= 8 or logits.dtype != torch.float32 or not logits.is_cuda:
        raise RuntimeError('label_map expects a [N,C,H,W] fp32 HIP tensor with 2 <= C <= 8')
    logits = logits.detach()
    if not logits.is_contiguous():
        logits = logits.contiguous()
    n, c, h, w = logits.shape
    out = torch.empty(n, h, w, device=logits.device, dtype=torch.int64)
    check(lib.aide_label_map(ptr(logits), c * h * w, c, n, h * w, ptr(out), stream_ptr()), 'label_map')
    return out


def predict_labels(net, *modal_inputs, **kw):
    """Labels [S,H,W] (int64, on device) for S slices; `modal_inputs` = (inphase[, outphase]) each
    [S,3,H,W].  The network must be in eval mode, as in the reference loop (:210 `net.eval()`).
    views='flip2' / 'flip4' / 'd4' or a tuple of view codes (aide_amd/ensemble.py): test-time augmentation -- every slice is
    predicted under each of the V views and the label is the first class of the largest mean soft-max (`ensemble_vote`);
    `net` may then be a list / tuple of networks of one class count that vote together (member i * V + j = network i under
    view j, at most 16 members, ValueError beyond), and a forward batch is V views of max(1, batch_size // V) slices.
    views=None (the default) with one network: the single identity forward and `label_map`, as before.
    window=wh or (wh, ww) (multiples of 16, the training size): sliding-window inference for slices of any H x W
    (aide_amd/window.py) -- windows at stride= (default: half the window), each forwarded (under every view, when views are
    given), their soft-max maps blended with window_weights= 'gaussian' (sigma_scale=0.125) or 'uniform'; the label is the first
    class of the largest blended probability, on the native grid.  stride / window_weights / sigma_scale without window:
    TypeError.  window=None (the default): every call takes the path it took before."""
    batch_size = kw.pop('batch_size', 16)
    views = kw.pop('views', None)
    win = _window_kw(kw)
    if kw:
        raise TypeError('unexpected arguments %r' % sorted(kw))
    if win is not None:
        return predict_windows(net, modal_inputs, views=views, batch_size=batch_size, **win)
    if views is not None or isinstance(net, (list, tuple)):
        return predict_ensemble(net, modal_inputs, (0,) if views is None else views, batch_size=batch_size)
    if net.training:
        raise RuntimeError('predict_labels needs net.eval(): train-mode BatchNorm at bs=1 is not what the '
                           'reference loop runs')
    s = modal_inputs[0].shape[0]
    dev = next(net.parameters()).device
    out = []
    with torch.no_grad():
        for i in range(0, s, batch_size):
            xs = [m[i:i + batch_size].to(dev, non_blocking=True) for m in modal_inputs]
            out.append(label_map(net(*xs)))
    return torch.cat(out, 0) if len(out) > 1 else out[0]


def _window_kw(kw):
    """pops window / stride / window_weights / sigma_scale -> the keywords of `predict_windows`, or None without a window"""
    given = sorted(k for k in ('stride', 'window_weights', 'sigma_scale') if k in kw)
    window = kw.pop('window', None)
    if window is None:
        if given:
            raise TypeError('%s go with window=' % ' / '.join(given))
        return None
    return dict(window=window, stride=kw.pop('stride', None), weights=kw.pop('window_weights', 'gaussian'),
                sigma_scale=kw.pop('sigma_scale', 0.125))


_UNSET = object()


def _target_grid(modal_inputs, spacing, target, windowed):
    """(H', W') of the slices at the in-plane spacing `target`, or None when that is the grid they are on"""
    try:
        t = tuple(float(v) for v in target)
    except TypeError:
        t = ()
    if len(t) != 2:
        raise ValueError('predict_case: target_spacing %r, two finite positive numbers (t_h, t_w) are expected' % (target,))
    s, _, h, w = modal_inputs[0].shape
    sp = _spacing(spacing, 'predict_case')
    (hn, wn, _), _ = resampled_shape((h, w, max(s, 1)), sp, t + sp[2:])
    if (hn, wn) == (h, w):
        return None
    if not windowed and (hn % 16 or wn % 16):
        raise ValueError('predict_case: the slices are %d x %d at target_spacing, not multiples of 16: pass window=' % (hn, wn))
    return hn, wn


def predict_case(net, *modal_inputs, **kw):
    """The reference's `generatedtarget`: numpy int64 [H,W,S] (slices stacked on the last axis, :267).
    keep_largest=True: its largest connected component (:268), uint8, filtered on the device before anything leaves it.
    keep_largest='per_class' with num_classes=C: the largest component of every class 1 .. C - 1 (`keep_largest_per_class`),
    uint8 class values, for multi-organ networks.
    numpy=False: the [H,W,S] HIP tensor instead (a permuted view of the [S,H,W] labels when unfiltered).
    views=...: the voted labels of `predict_labels(..., views=...)` (`net` may be a list of networks); probs=True then returns
    (volume, mean probabilities [S,C,H,W]) -- the probabilities are the vote's, before any filter.
    window= / stride= / window_weights= / sigma_scale=: the sliding-window labels of `predict_labels(..., window=...)`; with
    probs=True the probabilities are the blended ones [S,C,H,W]; the filters and fill_holes run on the blended labels.
    top_k= / min_voxels=: the filter `keep_largest` selects becomes `keep_components` with them (True: one slot; 'per_class':
    one per class, sequences allowed); TypeError when keep_largest is False.  fill_holes=True: `fill_holes` after the filter, on
    its uint8 output, binary or per class as the filter is (keep_largest=False: binary unless num_classes is given), along
    slice_axis= when given (2 is the slice axis of the [H,W,S] volume).  With all four at their defaults every call takes the
    path it took before.
    opening=r / closing=r (millimetres, with spacing=(sp_h, sp_w, sp_s), default 1 mm cubes; aide_amd/morphology.py): `open_`
    with the ball of radius r on the labels before the filter, `close` after fill_holes; both per class exactly when the filter
    is (keep_largest='per_class', or num_classes with no filter), binary otherwise.  spacing without either: TypeError.  With
    both at their defaults every call takes the path it took before.
    target_spacing=(t_h, t_w) (with spacing=; TypeError without it; aide_amd/resample.py): the in-plane spacing the network was
    trained at.  Every modal input is resampled per slice and channel to (H', W') = `resampled_shape` (order 1), the mean
    probabilities are predicted on that grid (views / lists of networks / window= compose; without window= an (H', W') that is
    not a multiple of 16 is a ValueError) and brought back to (S, H, W) with `resample_probs`: the labels, and with probs=True
    the probabilities, are the resampled ones, and opening, the filters, fill_holes and closing run on the native grid.
    (H', W') == (H, W) skips both resamples; target_spacing=None (the default): every call takes the path it took before."""
    keep_largest = kw.pop('keep_largest', False)
    want_probs = kw.pop('probs', False)
    num_classes = kw.pop('num_classes', None)
    as_numpy = kw.pop('numpy', True)
    top_k = kw.pop('top_k', _UNSET)               # (None is a value of its own: every blob that meets min_voxels)
    min_voxels = kw.pop('min_voxels', _UNSET)
    fill = kw.pop('fill_holes', False)
    slice_axis = kw.pop('slice_axis', None)
    opening = kw.pop('opening', None)
    closing = kw.pop('closing', None)
    spacing = kw.pop('spacing', None)
    target = kw.pop('target_spacing', None)
    morph = opening is not None or closing is not None
    if target is not None and spacing is None:
        raise TypeError('predict_case: target_spacing needs spacing=(sp_h, sp_w, sp_s)')
    if spacing is not None and not morph and target is None:
        raise TypeError('predict_case: spacing goes with opening / closing')
    per_class = isinstance(keep_largest, str)
    if per_class:
        if keep_largest != 'per_class':
            raise ValueError("keep_largest must be True, False or 'per_class', got %r" % (keep_largest,))
        if num_classes is None:
            raise TypeError("predict_case: keep_largest='per_class' needs num_classes")
        num_classes = classes(num_classes, 'predict_case', strict=False)
    elif num_classes is not None and (keep_largest or not (fill or morph)):
        raise TypeError("predict_case: num_classes goes with keep_largest='per_class' (or with fill_holes / opening / closing and no filter)")
    ranked = top_k is not _UNSET or min_voxels is not _UNSET
    if ranked and not keep_largest:
        raise TypeError('predict_case: top_k / min_voxels go with keep_largest')
    if fill not in (False, True):
        raise ValueError('predict_case: fill_holes must be False or True, got %r' % (fill,))
    if slice_axis is not None and not fill:
        raise TypeError('predict_case: slice_axis goes with fill_holes=True')
    pr = None
    native = None if target is None else _target_grid(modal_inputs, spacing, target, kw.get('window') is not None)
    if native is not None:
        first = net[0] if isinstance(net, (list, tuple)) else net
        dev = next(first.parameters()).device
        s, _, h, w = modal_inputs[0].shape
        modal_inputs = tuple(resample_image(m.to(dev).reshape(-1, 1, h, w), (1,) + native).reshape(tuple(m.shape[:2]) + native)
                             for m in modal_inputs)
    if want_probs or native is not None:
        views = kw.pop('views', None)
        batch_size = kw.pop('batch_size', 16)
        win = _window_kw(kw)
        if kw:
            raise TypeError('unexpected arguments %r' % sorted(kw))
        if win is not None:
            vol, pr = predict_windows(net, modal_inputs, views=views, batch_size=batch_size, probs=True, **win)
        else:
            vol, pr = predict_ensemble(net, modal_inputs, (0,) if views is None else views, batch_size=batch_size, probs=True)
        if native is not None:
            vol = resample_probs(pr, (s, h, w), probs_out=want_probs)
            vol, pr = vol if want_probs else (vol, None)
        vol = vol.permute(1, 2, 0)
    else:
        vol = predict_labels(net, *modal_inputs, **kw).permute(1, 2, 0)
    if opening is not None:
        vol = open_(vol, opening, (1.0, 1.0, 1.0) if spacing is None else spacing, num_classes)
    if ranked:
        vol = keep_components(vol, 1 if top_k is _UNSET else top_k, 1 if min_voxels is _UNSET else min_voxels,
                              num_classes if per_class else None)
    elif per_class:
        vol = keep_largest_per_class(vol, num_classes)
    elif keep_largest:
        vol = keep_largest_connected_components(vol)
    if fill:
        vol = fill_holes(vol, num_classes, slice_axis)
    if closing is not None:
        vol = close(vol, closing, (1.0, 1.0, 1.0) if spacing is None else spacing, num_classes)
    if not as_numpy:
        return vol if pr is None else (vol, pr)
    vol = vol.contiguous().cpu().numpy()
    return vol if pr is None else (vol, pr.cpu().numpy())


def Dice3d_fn(inputs, targets):
    """trainchaos_comparison_1case.py:88-95 for label volumes (numpy arrays or tensors): 2·Σ(i·t)/(Σi+Σt).
    Integer sums, one float64 division — identical to the numpy original (0/0 -> nan like numpy)."""
    if isinstance(inputs, np.ndarray) and isinstance(targets, np.ndarray):
        i, t = inputs.reshape(-1), targets.reshape(-1)
        return 2 * np.sum(i * t) / (np.sum(i) + np.sum(t))
    i = torch.as_tensor(inputs).reshape(-1).to(torch.int64)
    t = torch.as_tensor(targets).reshape(-1).to(i.device, torch.int64)
    inter, union = 2 * int((i * t).sum().item()), int(i.sum().item()) + int(t.sum().item())
    return np.float64(inter) / np.float64(union) if union else np.float64('nan')


# the argument checks alone, as tests/test_eval_host.py runs them on meta tensors
def _lcc_args(mask):
    volume_args(mask, 'keep_largest_connected_components')


def _confusion_args(pred, target):
    device_pair(pred, target, 'case_scores')


def _confusion_device(pred, target):
    """-> (N, sum P*T, sum P, sum T) as Python ints: one launch, one 32-byte device-to-host copy."""
    p, t = device_pair(pred, target.to(pred.device), 'case_scores')
    out = torch.empty(4, device=p.device, dtype=torch.int64)
    check(lib.aide_case_confusion(ptr(p), u8(p), *p.stride(), ptr(t), u8(t), *t.stride(), *p.shape, ptr(out), stream_ptr()),
          'case_confusion')
    return tuple(int(v) for v in out.cpu().tolist())


def _confusion_host(pred, target):
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    t = np.asarray(target).reshape(-1).astype(np.int64)
    if p.shape != t.shape:
        raise RuntimeError('case_scores: shape mismatch %s vs %s' % (np.shape(pred), np.shape(target)))
    return p.size, int(np.sum(p * t)), int(np.sum(p)), int(np.sum(t))


def _class_counts_device(pred, target, c):
    """-> counts[C,3] int64 (numpy): one launch, one copy of C * 3 int64"""
    p, t = device_pair(pred, target.to(pred.device), 'case_scores')
    out = torch.empty(c, 3, device=p.device, dtype=torch.int64)
    check(lib.aide_mc_counts_labels(ptr(p), u8(p), *p.stride(), ptr(t), u8(t), *t.stride(), *p.shape, c, ptr(out),
                                    stream_ptr()), 'mc_counts_labels')
    return out.cpu().numpy()


def _class_counts_host(pred, target, c):
    p, t = np.asarray(pred).reshape(-1), np.asarray(target).reshape(-1)
    if p.shape != t.shape:
        raise RuntimeError('case_scores: shape mismatch %s vs %s' % (np.shape(pred), np.shape(target)))
    out = np.zeros((c, 3), np.int64)
    for k in range(c):
        i, j = p == k, t == k
        out[k] = (i & j).sum(), i.sum(), j.sum()
    return out


def _case_scores_classes(pred, target, c):
    c = classes(c, 'case_scores', strict=False)
    dev = [x for x in (pred, target) if isinstance(x, torch.Tensor) and x.is_cuda]
    if dev:
        pred = torch.as_tensor(pred, device=dev[0].device)
        target = torch.as_tensor(target, device=dev[0].device)
        cnt = _class_counts_device(pred, target, c)
    else:
        pred, target = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (pred, target))
        cnt = _class_counts_host(pred, target, c)
    n = int(np.prod(np.shape(pred), dtype=np.int64))
    tp, si, st = cnt[:, 0], cnt[:, 1], cnt[:, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        dice = (2 * tp).astype(np.float64) / (si + st).astype(np.float64)
        iou = tp.astype(np.float64) / (si + st - tp).astype(np.float64)
    return dict(Dice=dice, IoU=iou, TP=tp.copy(), TN=n - si - st + tp, FP=si - tp, FN=st - tp)


def case_scores(pred, target, num_classes=None, spacing=None, percentiles=None, tolerances=None, lesions=None):
    """Per-case scores of the evaluation script (evalchaos_comparison_1cases.py:116-141, 238-242) for a predicted label
    volume against its target: dict(Dice, IoU, TP, TN, FP, FN).  HIP tensors: one confusion launch and one copy of four
    int64 sums to the host; anything else: the same sums in int64 on the CPU.  TP = sum p*t, FP = sum p - TP,
    FN = sum t - TP, TN = N - sum p - sum t + TP (the reference's formulas, exact for any integers); Dice = 2 TP /
    (sum p + sum t) and IoU = TP / (sum p + sum t - TP) as float64 true division like numpy's (0/0 -> nan, x/0 -> inf).
    num_classes=C (2 .. 8): the same six scores per class for multi-class label volumes, as arrays of [C] (Dice, IoU float64,
    the rest int64) with p_c = (pred == c), t_c = (target == c); a label outside [0, C) belongs to no class.  HIP tensors: one
    launch of aide_mc_counts_labels and one copy of C * 3 int64.
    spacing=(sp0, sp1, sp2), the edge lengths of a voxel along the three dims of the volumes (the evaluation script's
    `voxelspacing`, :181, 192-194): the dict also carries RAVD, ASSD and MSSD of `utils.metrics3d.surface_scores`; without it
    the dict is the six scores above and nothing else.
    percentiles=(q, ...) / tolerances=(tau, ...) (1 .. 4 numbers each; they need `spacing`, TypeError without it) go to
    `surface_scores` and add HD and HD_pooled ([Q], or [C, Q]) / NSD ([T], or [C, T]): percentiles=(95,) is HD95.
    lesions=overlap (a number in [0, 1]; 3-D volumes): the dict also carries the nine entries of `lesion_scores(pred, target,
    num_classes, overlap)`, each key prefixed `lesion_`.  With lesions=None every call takes the path it took without the
    argument and the dict has the keys it had."""
    if lesions is not None:
        overlap = _overlap(lesions, 'case_scores')
        res = case_scores(pred, target, num_classes, spacing, percentiles, tolerances)
        res.update(('lesion_' + k, v) for k, v in lesion_scores(pred, target, num_classes, overlap).items())
        return res
    if spacing is None and (percentiles is not None or tolerances is not None):
        raise TypeError('case_scores: percentiles / tolerances are surface distances and need spacing=(sp0, sp1, sp2)')
    if spacing is not None:
        from .utils.metrics3d import surface_scores
        res = case_scores(pred, target, num_classes)
        surf = surface_scores(pred, target, spacing, num_classes, percentiles=percentiles, tolerances=tolerances)
        res.update((k, surf[k]) for k in ('RAVD', 'ASSD', 'MSSD', 'HD', 'HD_pooled', 'NSD') if k in surf)
        return res
    if num_classes is not None:
        return _case_scores_classes(pred, target, num_classes)
    dev = [x for x in (pred, target) if isinstance(x, torch.Tensor) and x.is_cuda]
    if dev:
        pred = torch.as_tensor(pred, device=dev[0].device)
        target = torch.as_tensor(target, device=dev[0].device)
        n, spt, sp, st = _confusion_device(pred, target)
    else:
        n, spt, sp, st = _confusion_host(pred, target)
    with np.errstate(divide='ignore', invalid='ignore'):
        dice = np.float64(2 * spt) / np.float64(sp + st)
        iou = np.float64(spt) / np.float64(sp + st - spt)
    return dict(Dice=dice, IoU=iou, TP=spt, TN=n - sp - st + spt, FP=sp - spt, FN=st - spt)


# ---- all cases of an epoch at once (the epoch end of trainchaos_proposed_30cases1labeled.py:429-496) ----------------
def case_dice_rule(sums, labelled=None, n_select=0):
    """The host statement of `aide_label_refresh_select` (numpy): int64 sums [K,4] -> (dice float32 [K], rank int32 [K],
    selected uint8 [K]).  dice = float32(float64(2 * sum p*t) / float64(sum p + sum t)); rank and selected by `_rank_select`
    with every case that is not labelled eligible."""
    sums = np.asarray(sums, np.int64).reshape(-1, 4)
    with np.errstate(divide='ignore', invalid='ignore'):
        dice = (np.float64(2) * sums[:, 1].astype(np.float64) / (sums[:, 2] + sums[:, 3]).astype(np.float64)).astype(np.float32)
    rank, sel = _rank_select(dice, _unlabelled(labelled, len(dice)), n_select)
    return dice, rank, sel


def _unlabelled(labelled, k):
    return np.ones(k, bool) if labelled is None else ~np.asarray(labelled).astype(bool)


def _rank_select(dice, eligible, n_select):
    """THE ranking of every pseudo-label refresh, on the host: float32 scores [K] -> (rank int32 [K]: ascending, NaN greatest,
    equal values -- two NaNs included -- by the lower index; flag uint8 [K] = rank < n_select and eligible).  The tie rule is this
    project's, not parity: the reference's `Tensor.sort()` is not stable."""
    key = np.where(np.isnan(dice), np.float32(np.inf), dice)
    nan = np.isnan(dice).astype(np.int64)
    order = np.lexsort((np.arange(len(dice)), key, nan))          # last key first: NaN flag, value, index
    rank = np.empty(len(dice), np.int32)
    rank[order] = np.arange(len(dice), dtype=np.int32)
    return rank, ((rank < int(n_select)) & eligible).astype(np.uint8)


def _palette(palette, c, what):
    """the palette of a C-class bank as a tuple of C distinct bytes"""
    if palette is None:
        raise ValueError('%s: num_classes needs the palette (num_classes distinct bytes)' % what)
    pal = tuple(int(v) for v in palette)
    if len(pal) != c or len(set(pal)) != c or any(not 0 <= v <= 255 for v in pal):
        raise ValueError('%s: the palette must hold %d distinct bytes, got %r' % (what, c, pal))
    return pal


def _byte_classes(palette, none):
    """uint8 -> class table of a palette of distinct bytes; `none` for a byte outside it"""
    tbl = np.full(256, none, np.int64)
    tbl[np.asarray(palette, np.int64)] = np.arange(len(palette))
    return tbl


def case_class_counts(filtered, bank_plane, slice_start, palette):
    """The host statement of `aide_case_class_counts_batched` (numpy): label maps and one bank plane, both [S_total,H,W], of K
    concatenated cases -> int64 [K,C,3] with C = len(palette): row (k, c) = (#(f == c and b == palette[c]), #(f == c),
    #(b == palette[c])) over the slices of case k.  A predicted value >= C (or negative) and a bank byte outside the palette
    belong to no class."""
    f, b = np.asarray(filtered), np.asarray(bank_plane)
    if f.shape != b.shape:
        raise RuntimeError('case_class_counts: shape mismatch %s vs %s' % (f.shape, b.shape))
    c = len(palette)
    pal = _palette(palette, c, 'case_class_counts')
    st = _starts(slice_start, f.shape[0])
    cb = _byte_classes(pal, c)[b.astype(np.uint8)]
    cf = np.where((f >= 0) & (f < c), f, c).astype(np.int64)
    out = np.zeros((len(st) - 1, c, 3), np.int64)
    for k, (lo, hi) in enumerate(zip(st, st[1:])):
        x, y = cf[lo:hi].reshape(-1), cb[lo:hi].reshape(-1)
        out[k, :, 0] = np.bincount(x[x == y], minlength=c + 1)[:c]
        out[k, :, 1] = np.bincount(x, minlength=c + 1)[:c]
        out[k, :, 2] = np.bincount(y, minlength=c + 1)[:c]
    return out


def case_dice_rule_classes(counts, labelled=None, n_select=0):
    """The host statement of `aide_label_refresh_select_classes` (numpy): int64 counts [K,C,3] = (I, P, T) per case and class
    -> (class_dice float32 [K,C], dice float32 [K], rank int32 [K], selected uint8 [K]).  In float64 d_c = 2 I_c / (P_c + T_c)
    (0 / 0 -> NaN); class_dice = float32(d_c) for every class, background included.  The case score is the float64 mean of
    d_c over the FOREGROUND classes c = 1 .. C - 1 with P_c + T_c > 0 -- summed in ascending c, divided by their number,
    rounded once to float32 -- and NaN when there is none: an organ absent from the prediction and the pseudo-label alike
    says nothing about the case, one present in only one of them scores 0.  Ranking and selection are `case_dice_rule`'s.
    With C = 2 the score is one term over 1.0: the binary rule, bit for bit."""
    counts = np.asarray(counts, np.int64)
    if counts.ndim != 3 or counts.shape[2] != 3 or not 2 <= counts.shape[1] <= 8:
        raise RuntimeError('case_dice_rule_classes: counts [K,C,3] with C = 2 .. 8 expected, got %r' % (counts.shape,))
    k, c = counts.shape[:2]
    uni = counts[:, :, 1] + counts[:, :, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        d = (2 * counts[:, :, 0]).astype(np.float64) / uni.astype(np.float64)
    total, present = np.zeros(k, np.float64), np.zeros(k, np.int64)
    for j in range(1, c):                                         # the fixed order of the device sum
        has = uni[:, j] > 0
        total = np.where(has, total + np.where(has, d[:, j], 0.0), total)
        present += has
    with np.errstate(divide='ignore', invalid='ignore'):
        dice = (total / present.astype(np.float64)).astype(np.float32)        # no organ: 0 / 0, the NaN of the binary rule
    rank, sel = _rank_select(dice, _unlabelled(labelled, k), n_select)
    return d.astype(np.float32), dice, rank, sel


def _device_palette(palette, c, device):
    """the int32 HIP table of a C-class palette: the owner's own (it has checked the values), or one made from the bytes"""
    if isinstance(palette, torch.Tensor):
        if not (palette.is_cuda and palette.dtype == torch.int32 and palette.dim() == 1 and palette.numel() == c
                and palette.is_contiguous()):
            raise ValueError('evaluate_label_maps: a device palette must be a contiguous int32 HIP tensor [%d]' % c)
        return palette
    return torch.tensor(_palette(palette, c, 'evaluate_label_maps'), dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def evaluate_label_maps(labels, slice_start, bank_plane, match=63, labelled=None, n_select=0, keep_largest=True,
                        num_classes=None, palette=None):
    """Label maps [S_total,H,W] of K concatenated cases against one plane of the pseudo-label bank (uint8 [S_total,H,W]):
    dict(filtered uint8 [S_total,H,W], sums int64 [K,4] = N / sum p*t / sum p / sum t with t = (bank byte == match),
    dice float32 [K], rank int32 [K], selected uint8 [K]).  On HIP tensors eight launches, all results stay on the device and
    nothing synchronises; slice_start / labelled are then device tables (int64 [K+1] / uint8 [K]).  On numpy / CPU inputs the
    same integers through the CPU filter.
    num_classes=C (2 .. 8) with palette = C distinct bytes (ValueError otherwise; `match` is not used): the multi-organ form.
    The filter is `keep_largest_batched(num_classes=C)` (keep_largest=False: a plain uint8 cast either way), the result
    dict(filtered, counts int64 [K,C,3], class_dice float32 [K,C], dice, rank, selected) of `case_class_counts` and
    `case_dice_rule_classes`; on HIP tensors `aide_case_class_counts_batched` and `aide_label_refresh_select_classes`, with
    the same no-synchronisation rule (the palette may then be the int32 HIP table its owner keeps)."""
    c = None if num_classes is None else int(num_classes)
    if c is None and palette is not None:
        raise ValueError('evaluate_label_maps: palette goes with num_classes')
    if c is not None and not 2 <= c <= 8:
        raise ValueError('evaluate_label_maps: num_classes %d, 2 .. 8 are supported' % c)
    if isinstance(labels, torch.Tensor) and labels.is_cuda:
        pal = _device_palette(palette, c, labels.device) if c else None
        filt = keep_largest_batched(labels, slice_start, num_classes=c) if keep_largest else labels.to(torch.uint8).contiguous()
        if not (isinstance(bank_plane, torch.Tensor) and bank_plane.is_cuda and bank_plane.dtype == torch.uint8
                and bank_plane.is_contiguous() and tuple(bank_plane.shape) == tuple(filt.shape)):
            raise RuntimeError('evaluate_label_maps: bank_plane must be a contiguous uint8 HIP tensor shaped like the labels')
        k = slice_start.numel() - 1
        if labelled is not None and not (isinstance(labelled, torch.Tensor) and labelled.is_cuda
                                         and labelled.dtype == torch.uint8 and labelled.numel() == k):
            raise RuntimeError('evaluate_label_maps: labelled must be a uint8 HIP tensor [K]')
        dev = filt.device
        dice = torch.empty(k, device=dev, dtype=torch.float32)
        rank = torch.empty(k, device=dev, dtype=torch.int32)
        sel = torch.empty(k, device=dev, dtype=torch.uint8)
        out = (ptr(dice), ptr(rank), ptr(sel), stream_ptr())
        planes = (ptr(filt), ptr(bank_plane), ptr(slice_start), k) + tuple(filt.shape)
        lab = ptr(labelled) if labelled is not None else None
        if c:
            counts = torch.empty(k, c, 3, device=dev, dtype=torch.int64)
            cd = torch.empty(k, c, device=dev, dtype=torch.float32)
            check(lib.aide_case_class_counts_batched(*planes, ptr(pal), c, ptr(counts), stream_ptr()), 'case_class_counts_batched')
            check(lib.aide_label_refresh_select_classes(ptr(counts), lab, k, c, int(n_select), ptr(cd), *out),
                  'label_refresh_select_classes')
            return dict(filtered=filt, counts=counts, class_dice=cd, dice=dice, rank=rank, selected=sel)
        sums = torch.empty(k, 4, device=dev, dtype=torch.int64)
        check(lib.aide_case_confusion_batched(*planes, int(match), ptr(sums), stream_ptr()), 'case_confusion_batched')
        check(lib.aide_label_refresh_select(ptr(sums), lab, k, int(n_select), *out), 'label_refresh_select')
        return dict(filtered=filt, sums=sums, dice=dice, rank=rank, selected=sel)
    if c:
        pal = _palette(palette.tolist() if isinstance(palette, torch.Tensor) else palette, c, 'evaluate_label_maps')
    lab = np.asarray(labels)
    st = _starts(slice_start, lab.shape[0])
    filt = keep_largest_batched(lab, st, num_classes=c) if keep_largest else lab.astype(np.uint8)
    if c:
        counts = case_class_counts(filt, bank_plane, st, pal)
        cd, dice, rank, sel = case_dice_rule_classes(counts, labelled, n_select)
        return dict(filtered=filt, counts=counts, class_dice=cd, dice=dice, rank=rank, selected=sel)
    t = np.asarray(bank_plane) == match
    sums = np.zeros((len(st) - 1, 4), np.int64)
    for k, (a, b) in enumerate(zip(st, st[1:])):
        sums[k] = _confusion_host(filt[a:b], t[a:b])
    dice, rank, sel = case_dice_rule(sums, labelled, n_select)
    return dict(filtered=filt, sums=sums, dice=dice, rank=rank, selected=sel)


def evaluate_cases(net, modal_inputs, slice_start, bank_plane, match=63, batch_size=16, labelled=None, n_select=0,
                   num_classes=None, palette=None, views=None):
    """All cases of an epoch in one pass: `modal_inputs` = (inphase[, outphase]), each [S_total,3,H,W] with the slices of the
    K cases concatenated.  The forward batches may cross case boundaries (eval-mode BatchNorm: slices are independent);
    filter, sums, Dice and ranking are `evaluate_label_maps` (num_classes / palette: its multi-organ form, for a C-class
    network).  views: the test-time augmentation of `predict_labels` (None: the single forward).  Nothing leaves the device."""
    labels = predict_labels(net, *modal_inputs, batch_size=batch_size, views=views)
    return evaluate_label_maps(labels, slice_start, bank_plane, match=match, labelled=labelled, n_select=n_select,
                               num_classes=num_classes, palette=palette)


# ---- all IMAGES of an epoch (the epoch end of trainkidney_proposed_mask1.py:373-434 and
# trainbreast_dataset3_proposed_272cases25labeled.py:373-438) -------------------------------------------------------------
MAX_IMAGES = 1 << 20


def image_dice_rule(sums, labelled=None, n_select=0):
    """The host statement of `aide_image_refresh_select` (numpy): int64 sums [K,4] -> (dice float32 [K], rank int32 [K],
    written uint8 [K]).  dice = 0.0 where sum p + sum t == 0 (Dice2d, :137-138: never NaN), else float32(float64(2 * sum p*t)
    / float64(sum p + sum t)); rank and written by `_rank_select`, an image being eligible when sum p > 0 (:418 `if
    save_data.sum() > 0`) and it is not labelled."""
    sums = np.asarray(sums, np.int64).reshape(-1, 4)
    uni = sums[:, 2] + sums[:, 3]
    dice = np.zeros(len(sums), np.float32)
    nz = uni != 0
    dice[nz] = ((2 * sums[nz, 1]).astype(np.float64) / uni[nz].astype(np.float64)).astype(np.float32)
    rank, written = _rank_select(dice, (sums[:, 2] > 0) & _unlabelled(labelled, len(dice)), n_select)
    return dice, rank, written


def _image_eval_args(what, src, score_rows, gate, k0, pred, sums):
    n, (h, w) = src.shape[0], src.shape[-2:]
    k = pred.shape[0]
    ok = (src.is_cuda and src.is_contiguous() and score_rows.is_cuda and score_rows.dtype == torch.uint8
          and score_rows.is_contiguous() and tuple(score_rows.shape) == (n, h, w)
          and pred.is_cuda and pred.dtype == torch.uint8 and pred.is_contiguous() and tuple(pred.shape) == (k, h, w)
          and sums.is_cuda and sums.dtype == torch.int64 and sums.is_contiguous() and tuple(sums.shape) == (k, 4)
          and (gate is None or (gate.is_cuda and gate.dtype == torch.uint8 and gate.is_contiguous() and gate.numel() == k))
          and 0 <= k0 and k0 + n <= k <= MAX_IMAGES)
    if not ok:
        raise RuntimeError('%s: contiguous HIP tensors expected: score_rows uint8 [N,H,W], pred uint8 [K,H,W], sums int64 [K,4], '
                           'gate uint8 [K] or None, k0 + N <= K <= 2^20' % what)
    return n, h, w, k


def image_eval_logits(logits, score_rows, gate, k0, pred, sums):
    """The fused epilogue of a forward batch: logits [N,2,H,W] fp32 of the images k0 .. k0 + N - 1 -> pred[k0:k0 + N] =
    `label_map(logits)` as uint8 and sums[k0:k0 + N] = (H*W, sum p*t, sum p, sum t) with t = (score_rows > 0) & gate.  No int64
    label tensor exists at any point; nothing synchronises."""
    if logits.dim() != 4 or logits.shape[1] != 2 or logits.dtype != torch.float32:
        raise RuntimeError('image_eval_logits expects [N,2,H,W] fp32 logits')
    logits = logits.detach()
    if not logits.is_contiguous():
        logits = logits.contiguous()
    n, h, w, k = _image_eval_args('image_eval_logits', logits, score_rows, gate, k0, pred, sums)
    check(lib.aide_image_eval_logits(ptr(logits), 2 * h * w, ptr(score_rows), ptr(gate) if gate is not None else None, n, h, w,
                                     int(k0), k, ptr(pred), ptr(sums), stream_ptr()), 'image_eval_logits')


def image_eval_labels(labels, score_rows, gate, k0, pred, sums):
    """... from ready label maps [N,H,W] (uint8 or int64; p = label != 0), for `ImageLabelBank.refresh_from_labels`."""
    if labels.dim() != 3 or labels.dtype not in (torch.uint8, torch.int64):
        raise RuntimeError('image_eval_labels expects [N,H,W] uint8 or int64 label maps')
    labels = labels.detach()
    if not labels.is_contiguous():
        labels = labels.contiguous()
    n, h, w, k = _image_eval_args('image_eval_labels', labels, score_rows, gate, k0, pred, sums)
    check(lib.aide_image_eval_labels(ptr(labels), int(labels.dtype == torch.uint8), ptr(score_rows),
                                     ptr(gate) if gate is not None else None, n, h, w, int(k0), k, ptr(pred), ptr(sums),
                                     stream_ptr()), 'image_eval_labels')


def image_refresh_select(sums, labelled=None, n_select=0, out=None):
    """int64 sums [K,4] on the device -> (dice float32 [K], rank int32 [K], written uint8 [K]) by `image_dice_rule`, for K up to
    2^20: two launches, no host read.  out: the three tensors to fill."""
    if not (sums.is_cuda and sums.dtype == torch.int64 and sums.dim() == 2 and sums.shape[1] == 4 and sums.is_contiguous()):
        raise RuntimeError('image_refresh_select: sums must be a contiguous int64 HIP tensor [K,4]')
    k = sums.shape[0]
    if k > MAX_IMAGES:
        raise RuntimeError('image_refresh_select: %d images, at most 2^20' % k)
    if labelled is not None and not (labelled.is_cuda and labelled.dtype == torch.uint8 and labelled.is_contiguous()
                                     and labelled.numel() == k):
        raise RuntimeError('image_refresh_select: labelled must be a uint8 HIP tensor [K]')
    if out is None:
        out = (torch.empty(k, device=sums.device, dtype=torch.float32), torch.empty(k, device=sums.device, dtype=torch.int32),
               torch.empty(k, device=sums.device, dtype=torch.uint8))
    dice, rank, written = out
    for t, dt in ((dice, torch.float32), (rank, torch.int32), (written, torch.uint8)):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == k):
            raise RuntimeError('image_refresh_select: out = (float32 [K], int32 [K], uint8 [K]) contiguous HIP tensors')
    check(lib.aide_image_refresh_select(ptr(sums), ptr(labelled) if labelled is not None else None, k, int(n_select), ptr(dice),
                                        ptr(rank), ptr(written), stream_ptr()), 'image_refresh_select')
    return dice, rank, written


def image_bank_update(pred, written, scale, plane):
    """plane[k] = pred[k] * scale where written[k] (uint8 [K,H,W] planes, `written` read on the device)."""
    ok = (pred.is_cuda and plane.is_cuda and written.is_cuda and pred.dtype == plane.dtype == written.dtype == torch.uint8
          and pred.dim() == 3 and pred.shape == plane.shape and pred.is_contiguous() and plane.is_contiguous()
          and written.is_contiguous() and written.numel() == pred.shape[0] <= MAX_IMAGES)
    if not ok:
        raise RuntimeError('image_bank_update: contiguous uint8 HIP tensors pred / plane [K,H,W] and written [K] expected')
    check(lib.aide_image_bank_update(ptr(pred), ptr(written), *pred.shape, int(scale), ptr(plane), stream_ptr()), 'image_bank_update')
