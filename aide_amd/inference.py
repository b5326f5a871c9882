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
    both at their defaults every call takes the path it took before."""
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
    morph = opening is not None or closing is not None
    if spacing is not None and not morph:
        raise TypeError('predict_case: spacing goes with opening / closing')
    per_class = isinstance(keep_largest, str)
    if per_class:
        if keep_largest != 'per_class':
            raise ValueError("keep_largest must be True, False or 'per_class', got %r" % (keep_largest,))
        if num_classes is None:
            raise TypeError("predict_case: keep_largest='per_class' needs num_classes")
        num_classes = _num_classes(num_classes, 'predict_case')
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
    if want_probs:
        views = kw.pop('views', None)
        batch_size = kw.pop('batch_size', 16)
        win = _window_kw(kw)
        if kw:
            raise TypeError('unexpected arguments %r' % sorted(kw))
        if win is not None:
            vol, pr = predict_windows(net, modal_inputs, views=views, batch_size=batch_size, probs=True, **win)
        else:
            vol, pr = predict_ensemble(net, modal_inputs, (0,) if views is None else views, batch_size=batch_size, probs=True)
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


def keep_largest_connected_components(mask):
    """trainchaos_comparison_1case.py:68-77 / trainchaos_proposed_30cases1labeled.py:103-112: the largest connected blob of a
    label volume (connectivity 1: face neighbours), uint8.  CPU post-processing in the reference (skimage.measure.label +
    regionprops).  skimage connects neighbours of EQUAL value (0 = background) and numbers the blobs in raster order of
    their first voxel; scipy.ndimage.label connects every non-zero voxel, so it is run once per label value and the blobs
    are ordered by their first voxel -- the same blob as the reference's `np.argmax(area)` on ties, and for a multi-class
    volume (num_classes up to 8 here) blobs of different classes stay separate as they do there."""
    if isinstance(mask, torch.Tensor) and mask.is_cuda:
        return _keep_largest_device(mask)
    from scipy import ndimage
    mask = np.asarray(mask)
    out = np.zeros(mask.shape, dtype=np.uint8)
    if mask.size == 0 or mask.max() <= 0:
        return out
    best = None                                   # (area, -first voxel, value, blob labels, blob id)
    for v in np.unique(mask):
        if v == 0:
            continue
        blobs, count = ndimage.label(mask == v)
        flat = blobs.reshape(-1)
        area = np.bincount(flat, minlength=count + 1)[1:]
        first = np.full(count + 1, flat.size, dtype=np.int64)
        idx = np.flatnonzero(flat)
        np.minimum.at(first, flat[idx], idx)
        for b in range(count):
            cand = (int(area[b]), -int(first[b + 1]))
            if best is None or cand > best[0]:
                best = (cand, blobs, b + 1)
    out[best[1] == best[2]] = 1
    return out


_MAX_VOX = 2 ** 31 - 1
_INT_DTYPES = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool)


def _lcc_args(mask):
    """Argument checks of the device filter (before anything is launched): a 3-D integer tensor of < 2^31 voxels."""
    if mask.dim() != 3:
        raise RuntimeError('keep_largest_connected_components: a 3-D volume is expected, got %d dims' % mask.dim())
    if mask.dtype not in _INT_DTYPES:
        raise RuntimeError('keep_largest_connected_components: integer labels expected, got %s' % mask.dtype)
    if mask.numel() > _MAX_VOX:
        raise RuntimeError('keep_largest_connected_components: %d voxels, at most 2^31 - 1' % mask.numel())


def _keep_largest_device(mask):
    """HIP tensor (d0, d1, d2) of integer labels, any strides -> uint8 HIP tensor of the same shape (1 on the largest
    blob); raster order is C order of the LOGICAL index.  Asynchronous: no host synchronisation."""
    _lcc_args(mask)
    mask = mask.detach()
    if mask.dtype != torch.int64:
        mask = mask.to(torch.int64)
    out = torch.empty(mask.shape, device=mask.device, dtype=torch.uint8)
    if mask.numel() == 0:
        return out
    ws = torch.empty(lib.aide_lcc3d_ws_bytes(mask.numel()), device=mask.device, dtype=torch.uint8)
    check(lib.aide_keep_largest_cc3d(ptr(mask), *mask.shape, *mask.stride(), ptr(out), ptr(ws), stream_ptr()),
          'keep_largest_cc3d')
    return out


def _num_classes(c, what):
    c = int(c)
    if not 2 <= c <= 8:
        raise RuntimeError('%s: num_classes %d, 2 .. 8 are supported' % (what, c))
    return c


def keep_largest_per_class(mask, num_classes, stats=False):
    """The filter for multi-organ volumes (the reference has one blob for the whole volume, which keeps the liver of a CHAOS
    prediction and deletes the kidneys and the spleen): for every class value c in 1 .. num_classes - 1 the largest blob of
    the voxels equal to c (connectivity 1; a tie goes to the blob whose first voxel comes first in raster order of the logical
    index, the rule of `keep_largest_connected_components` per class).  uint8 volume of the same shape: c on the kept blob
    of class c, 0 elsewhere; a value outside 1 .. num_classes - 1 belongs to no class; a class that does not occur leaves
    nothing.  num_classes = 2 on a {0, 1} volume is `keep_largest_connected_components`, byte for byte.
    stats=True: also int64 [num_classes, 3], row c = (blobs of class c, voxels of class c, voxels of the kept blob), row 0
    zeros.  HIP integer tensor of any strides: `aide_keep_largest_cc3d_classes`, five launches and one memset, asynchronous,
    HIP tensors returned.  numpy array or CPU tensor: scipy.ndimage.label once per class, numpy arrays returned."""
    c = _num_classes(num_classes, 'keep_largest_per_class')
    if isinstance(mask, torch.Tensor) and mask.is_cuda:
        out, st = _keep_largest_classes_device(mask, c, stats)
    else:
        if isinstance(mask, torch.Tensor):
            mask = mask.detach().numpy()
        out, st = _keep_largest_classes_host(np.asarray(mask), c)
    return (out, st) if stats else out


def _keep_largest_classes_host(mask, c):
    from scipy import ndimage
    out = np.zeros(mask.shape, dtype=np.uint8)
    st = np.zeros((c, 3), dtype=np.int64)
    if mask.size == 0:
        return out, st
    for v in range(1, c):
        blobs, count = ndimage.label(mask == v)
        if count == 0:
            continue
        flat = blobs.reshape(-1)
        area = np.bincount(flat, minlength=count + 1)[1:]
        first = np.full(count + 1, flat.size, dtype=np.int64)
        idx = np.flatnonzero(flat)
        np.minimum.at(first, flat[idx], idx)
        b = max(range(count), key=lambda j: (int(area[j]), -int(first[j + 1])))
        out[blobs == b + 1] = v
        st[v] = count, int(area.sum()), int(area[b])
    return out, st


def _keep_largest_classes_device(mask, c, stats):
    _lcc_args(mask)
    mask = mask.detach()
    if mask.dtype != torch.int64:
        mask = mask.to(torch.int64)
    out = torch.empty(mask.shape, device=mask.device, dtype=torch.uint8)
    st = torch.empty(c, 3, device=mask.device, dtype=torch.int64) if stats else None
    if mask.numel() == 0:
        return out, (st.zero_() if stats else None)
    ws = torch.empty(lib.aide_lcc3d_classes_ws_bytes(mask.numel(), c), device=mask.device, dtype=torch.uint8)
    check(lib.aide_keep_largest_cc3d_classes(ptr(mask), *mask.shape, *mask.stride(), c, ptr(out), ptr(st), ptr(ws),
                                             stream_ptr()), 'keep_largest_cc3d_classes')
    return out, st


# ---- case post-processing: the k largest blobs with a size floor, hole filling ------------------------------------------
MAX_TOP_K = 8


def _post_classes(num_classes, what):
    if num_classes is None:
        return None
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 2 <= num_classes <= 8:
        raise ValueError('%s: num_classes %r, None or 2 .. 8 are supported' % (what, num_classes))
    return int(num_classes)


def _per_class(value, c, name, check):
    """`value` (one entry, or with num_classes=c a sequence of c entries, entry 0 ignored) -> list of 8 checked entries"""
    if isinstance(value, (list, tuple, np.ndarray)):
        if c is None or len(value) != c:
            raise ValueError('keep_components: a sequence for %s needs num_classes and one entry per class value, got %r'
                             % (name, value))
        vals = [check(v) for v in list(value)[1:]]
    else:
        vals = [check(value)] * ((c or 2) - 1)
    return [0] + vals + [vals[0]] * (8 - 1 - len(vals))


def _top_k(k):
    if k is None:
        return 0
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_TOP_K:
        raise ValueError('keep_components: top_k %r, None or 1 .. %d are supported' % (k, MAX_TOP_K))
    return int(k)


def _min_voxels(m):
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m < 1:
        raise ValueError('keep_components: min_voxels %r, an integer >= 1 is expected' % (m,))
    return min(int(m), 2 ** 31)


def _blobs_of(mask, v):
    """(labels, areas, first raster index) of the face-connected blobs of mask == v, one row per blob"""
    from scipy import ndimage
    blobs, count = ndimage.label(mask == v)
    flat = blobs.reshape(-1)
    area = np.bincount(flat, minlength=count + 1)[1:]
    first = np.full(count + 1, flat.size, dtype=np.int64)
    idx = np.flatnonzero(flat)
    np.minimum.at(first, flat[idx], idx)
    return blobs, area, first[1:]


def _keep_components_host(mask, c, ks, ms):
    """the host statement of aide_keep_components3d: scipy.ndimage.label once per value"""
    out = np.zeros(mask.shape, dtype=np.uint8)
    st = np.zeros((c or 2, 3), dtype=np.int64)
    if mask.size == 0 or (c is None and mask.max() <= 0):
        return out, st
    slots = [(v, [v]) for v in range(1, c)] if c else [(1, [v for v in np.unique(mask).tolist() if v != 0])]
    for cls, values in slots:
        found = []                                # (-area, first voxel, index into labelled, blob id)
        labelled = []
        for v in values:
            blobs, area, first = _blobs_of(mask, v)
            labelled.append((blobs, len(area)))
            found += [(-int(a), int(f), len(labelled) - 1, b + 1) for b, (a, f) in enumerate(zip(area, first))]
        found.sort()
        kept = [f for f in (found[:ks[cls]] if ks[cls] else found) if -f[0] >= ms[cls]]
        for j, (blobs, count) in enumerate(labelled):
            lut = np.zeros(count + 1, bool)
            lut[[f[3] for f in kept if f[2] == j]] = True
            out[lut[blobs]] = cls
        st[cls] = len(found), -sum(f[0] for f in found), -sum(f[0] for f in kept)
    return out, st


def keep_components(volume, top_k=1, min_voxels=1, num_classes=None, stats=False):
    """The component rule of `keep_largest_connected_components` / `keep_largest_per_class` with a rank and a size floor.
    Face neighbours of equal value are connected.  num_classes=None: one slot over all non-zero values, 1 is written (nothing
    when no value is positive, as the binary filter).  num_classes=C (2 .. 8): one slot per class value 1 .. C - 1, the class
    value is written; a value outside 1 .. C - 1 belongs to no class.  Inside a slot larger blobs come first and a tie goes to
    the blob whose first voxel has the lower raster index of the logical volume; kept are the first `top_k` blobs of that
    order (1 .. 8, or None for all), and of those the ones with at least `min_voxels` (>= 1) voxels.  With num_classes=C both
    may be sequences of C entries, one per class value, entry 0 ignored: top_k=(0, 1, 2) keeps one liver and two kidneys.
    Anything else raises ValueError before a launch.  top_k=1, min_voxels=1 is the two existing filters byte for byte.
    stats=True (with num_classes=C; TypeError without): also int64 [C, 3], row c = (blobs of class c, voxels of class c, voxels
    kept), row 0 zeros.  HIP integer tensor of any strides: `aide_keep_components3d`, 4 + max(1, top_k) launches, asynchronous,
    HIP tensors returned.  numpy array or CPU tensor: scipy.ndimage.label once per value, numpy arrays returned."""
    c = _post_classes(num_classes, 'keep_components')
    if stats and c is None:
        raise TypeError('keep_components: stats needs num_classes')
    ks = _per_class(top_k, c, 'top_k', _top_k)
    ms = _per_class(min_voxels, c, 'min_voxels', _min_voxels)
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        import ctypes
        _lcc_args(volume)
        v = volume.detach()
        if v.dtype != torch.int64:
            v = v.to(torch.int64)
        out = torch.empty(v.shape, device=v.device, dtype=torch.uint8)
        st = torch.empty(c, 3, device=v.device, dtype=torch.int64) if stats else None
        if v.numel() == 0:
            return (out, st.zero_()) if stats else out
        ws = torch.empty(lib.aide_components3d_ws_bytes(v.numel()), device=v.device, dtype=torch.uint8)
        check(lib.aide_keep_components3d(ptr(v), *v.shape, *v.stride(), c or 0, (ctypes.c_int * 8)(*ks),
                                         (ctypes.c_longlong * 8)(*ms), ptr(out), ptr(st), ptr(ws), stream_ptr()),
              'keep_components3d')
        return (out, st) if stats else out
    if isinstance(volume, torch.Tensor):
        volume = volume.detach().numpy()
    out, st = _keep_components_host(np.asarray(volume), c, ks, ms)
    return (out, st) if stats else out


def _fill_holes_host(vol, c, axis):
    """the host statement of aide_fill_holes3d: scipy.ndimage.label of the background (no links along `axis`), then per blob
    the set of things it touches"""
    from scipy import ndimage
    rows = c or 2
    st = np.zeros((rows, 2), dtype=np.int64)
    cls = np.where((vol >= 1) & (vol < c), vol, 0).astype(np.uint8) if c else (vol != 0).astype(np.uint8)
    if vol.size == 0:
        return cls, st
    link = ndimage.generate_binary_structure(3, 1)
    axes = [a for a in range(3) if a != axis]
    if axis is not None:
        link = link.copy()
        index = [1, 1, 1]
        for end in (0, 2):
            index[axis] = end
            link[tuple(index)] = False
    blobs, count = ndimage.label(vol == 0, structure=link)
    touch = np.zeros(count + 1, np.int64)         # bit 0: open or next to an out-of-range value, bit c: next to class c
    for a in axes:
        for end in (0, -1):
            touch[np.unique(np.take(blobs, end, axis=a))] |= 1
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        for here, there in ((tuple(lo), tuple(hi)), (tuple(hi), tuple(lo))):
            sel = (blobs[here] != 0) & (vol[there] != 0)
            np.bitwise_or.at(touch, blobs[here][sel], np.int64(1) << cls[there][sel].astype(np.int64) if c else 0)
    touch[0] = 1
    single = (touch & 1) == 0 if not c else (touch > 1) & (touch & (touch - 1) == 0)
    fill = np.zeros(count + 1, np.uint8)
    fill[single] = np.log2(touch[single]).astype(np.uint8) if c else 1
    out = np.where(blobs != 0, fill[blobs], cls).astype(np.uint8)
    area = np.bincount(blobs.reshape(-1), minlength=count + 1)
    for k in range(1, rows):
        st[k] = int((fill == k).sum()), int(area[fill == k].sum())
    return out, st


def fill_holes(volume, num_classes=None, slice_axis=None, stats=False):
    """Fill the enclosed cavities of a label volume.  Background is the voxels with value exactly 0; a hole is a face-connected
    blob of background with no voxel on a face of the volume.  slice_axis=a (0, 1 or 2): connectivity is restricted to the
    2-D slices along axis a and "face of the volume" reads "edge of the slice", the usual rule for anisotropic stacks
    (`predict_case`'s [H,W,S] volumes: slice_axis=2).
    num_classes=None: uint8, 1 where volume != 0 or the voxel lies in a hole: `scipy.ndimage.binary_fill_holes(volume != 0)`,
    applied per slice with a slice axis.  num_classes=C (2 .. 8): a voxel of class 1 .. C - 1 keeps its value, a value outside
    0 .. C - 1 is written as 0, and a hole is filled with class c if and only if every non-background face neighbour of the
    hole has value c, 1 <= c <= C - 1: a hole that touches two classes, or an out-of-range value, stays 0.  C = 2 on a {0, 1}
    volume is the binary result.  ValueError for any other num_classes or slice_axis.
    stats=True: also int64 [C, 2] (binary: [2, 2], row 1), row c = (holes filled with c, voxels filled with c), row 0 zeros.
    HIP tensor, int64 or uint8 (other integer types are widened), any strides: `aide_fill_holes3d`, five launches, asynchronous,
    HIP tensors returned.  numpy array or CPU tensor: scipy.ndimage.label of the background, numpy arrays returned."""
    c = _post_classes(num_classes, 'fill_holes')
    if slice_axis is not None and (isinstance(slice_axis, bool) or not isinstance(slice_axis, (int, np.integer))
                                   or not 0 <= slice_axis <= 2):
        raise ValueError('fill_holes: slice_axis %r, None, 0, 1 or 2 are supported' % (slice_axis,))
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        _lcc_args(volume)
        v = volume.detach()
        if v.dtype not in (torch.int64, torch.uint8):
            v = v.to(torch.int64)
        out = torch.empty(v.shape, device=v.device, dtype=torch.uint8)
        st = torch.empty(c or 2, 2, device=v.device, dtype=torch.int64) if stats else None
        if v.numel() == 0:
            return (out, st.zero_()) if stats else out
        ws = torch.empty(lib.aide_fill_holes3d_ws_bytes(v.numel()), device=v.device, dtype=torch.uint8)
        check(lib.aide_fill_holes3d(ptr(v), int(v.dtype == torch.uint8), *v.shape, *v.stride(), c or 0,
                                    -1 if slice_axis is None else int(slice_axis), ptr(out), ptr(st), ptr(ws), stream_ptr()),
              'fill_holes3d')
        return (out, st) if stats else out
    if isinstance(volume, torch.Tensor):
        volume = volume.detach().numpy()
    volume = np.asarray(volume)
    if volume.ndim != 3:
        raise RuntimeError('fill_holes: a 3-D volume is expected, got %d dims' % volume.ndim)
    out, st = _fill_holes_host(volume, c, None if slice_axis is None else int(slice_axis))
    return (out, st) if stats else out


def _confusion_args(pred, target):
    """Argument checks of the device scores: integer volumes (int64 or uint8 here; other integer types are widened) of
    the same shape, 1 to 3 dims (more are flattened into the first), < 2^31 voxels."""
    if tuple(pred.shape) != tuple(target.shape):
        raise RuntimeError('case_scores: shape mismatch %s vs %s' % (tuple(pred.shape), tuple(target.shape)))
    if pred.dim() == 0:
        raise RuntimeError('case_scores: volumes of at least one dim expected')
    for x in (pred, target):
        if x.dtype not in _INT_DTYPES:
            raise RuntimeError('case_scores: integer volumes expected, got %s' % x.dtype)
    if pred.numel() > _MAX_VOX:
        raise RuntimeError('case_scores: %d voxels, at most 2^31 - 1' % pred.numel())


def _as3d(x):
    x = x.detach()
    if x.dtype not in (torch.int64, torch.uint8):
        x = x.to(torch.int64)
    if x.dim() > 3:
        x = x.reshape((-1,) + tuple(x.shape[-2:]))
    while x.dim() < 3:
        x = x.unsqueeze(0)
    return x


def _confusion_device(pred, target):
    """-> (N, sum P*T, sum P, sum T) as Python ints: one launch, one 32-byte device-to-host copy."""
    _confusion_args(pred, target)
    p, t = _as3d(pred), _as3d(target.to(pred.device))
    out = torch.empty(4, device=p.device, dtype=torch.int64)
    check(lib.aide_case_confusion(ptr(p), int(p.dtype == torch.uint8), *p.stride(), ptr(t), int(t.dtype == torch.uint8),
                                  *t.stride(), *p.shape, ptr(out), stream_ptr()), 'case_confusion')
    return tuple(int(v) for v in out.cpu().tolist())


def _confusion_host(pred, target):
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    t = np.asarray(target).reshape(-1).astype(np.int64)
    if p.shape != t.shape:
        raise RuntimeError('case_scores: shape mismatch %s vs %s' % (np.shape(pred), np.shape(target)))
    return p.size, int(np.sum(p * t)), int(np.sum(p)), int(np.sum(t))


def _class_counts_device(pred, target, c):
    """-> counts[C,3] int64 (numpy): one launch, one copy of C * 3 int64"""
    _confusion_args(pred, target)
    p, t = _as3d(pred), _as3d(target.to(pred.device))
    out = torch.empty(c, 3, device=p.device, dtype=torch.int64)
    check(lib.aide_mc_counts_labels(ptr(p), int(p.dtype == torch.uint8), *p.stride(), ptr(t), int(t.dtype == torch.uint8),
                                    *t.stride(), *p.shape, c, ptr(out), stream_ptr()), 'mc_counts_labels')
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
    if not 2 <= c <= 8:
        raise RuntimeError('case_scores: num_classes %d, 2 .. 8 are supported' % c)
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
        return _case_scores_classes(pred, target, int(num_classes))
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


# ---- labelled components and lesion-wise detection scores ---------------------------------------------------------------
MAX_BLOBS = 2 ** 20
PROPS_COLUMNS = ('value', 'area', 'first', 'min0', 'min1', 'min2', 'max0', 'max1', 'max2', 'sum0', 'sum1', 'sum2')
LESION_COLUMNS = ('target_blobs', 'detected', 'pred_blobs', 'matched', 'covered_voxels', 'spurious_voxels')


def _max_blobs(m):
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= MAX_BLOBS:
        raise ValueError('label_components: max_blobs %r, an integer in 1 .. 2^20 is expected' % (m,))
    return int(m)


def _overlap(x, what='lesion_scores'):
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not 0.0 <= float(x) <= 1.0:
        raise ValueError('%s: overlap %r, a number in [0, 1] is expected' % (what, x))
    return float(x)


def _host_volume(x, what):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.ndim != 3:
        raise RuntimeError('%s: a 3-D volume is expected, got %d dims' % (what, x.ndim))
    if x.dtype != np.bool_ and not np.issubdtype(x.dtype, np.integer):
        raise RuntimeError('%s: integer labels expected, got %s' % (what, x.dtype))
    return x


def _label_host(vol, c):
    """-> (labels int32, value[n], area[n], first[n]): scipy.ndimage.label once per member value, the blobs of all values
    then ordered by their first voxel, computed explicitly"""
    labels = np.zeros(vol.shape, np.int32)
    empty = np.zeros(0, np.int64)
    if vol.size == 0:
        return labels, empty, empty, empty
    values = range(1, c) if c else [v for v in np.unique(vol).tolist() if v != 0]
    found = [(v,) + _blobs_of(vol, v) for v in values]
    value = np.concatenate([np.full(len(a), v, np.int64) for v, _, a, _ in found] + [empty])
    area = np.concatenate([a for _, _, a, _ in found] + [empty]).astype(np.int64)
    first = np.concatenate([f for _, _, _, f in found] + [empty]).astype(np.int64)
    order = np.argsort(first, kind='stable')      # (first voxels are distinct)
    number = np.empty(len(order), np.int64)
    number[order] = np.arange(1, len(order) + 1)
    at = 0
    for _, blobs, a, _ in found:
        lut = np.concatenate([[0], number[at:at + len(a)]]).astype(np.int32)
        labels += lut[blobs]                      # the blobs of different values do not overlap
        at += len(a)
    return labels, value[order], area[order], first[order]


def _props_host(labels, value, area, first, cap):
    props = np.zeros((cap, 12), np.int64)
    k = min(len(value), cap)
    props[:k, 0], props[:k, 1], props[:k, 2] = value[:k], area[:k], first[:k]
    flat = labels.reshape(-1)
    idx = np.flatnonzero((flat > 0) & (flat <= k))
    if not len(idx):
        return props
    order = np.argsort(flat[idx], kind='stable')  # the voxels blob by blob, every blob a run
    idx = idx[order]
    blob = flat[idx].astype(np.int64) - 1
    starts = np.flatnonzero(np.concatenate([[True], blob[1:] != blob[:-1]]))
    rows = blob[starts]
    for axis, x in enumerate(np.unravel_index(idx, labels.shape)):
        x = x.astype(np.int64)
        props[rows, 3 + axis] = np.minimum.reduceat(x, starts)
        props[rows, 6 + axis] = np.maximum.reduceat(x, starts) + 1
        props[rows, 9 + axis] = np.add.reduceat(x, starts)
    return props


def label_components(volume, num_classes=None, props=False, max_blobs=65536):
    """The label image of a volume and its region table: what the reference gets from skimage.measure.label(v, connectivity=1)
    and regionprops (evalchaos_comparison_1cases.py:72-81).  volume: a 3-D integer volume of fewer than 2^31 voxels, any
    strides.  num_classes=None: every voxel whose value is not 0 is a member; num_classes=C (2 .. 8): the values 1 .. C - 1
    are, anything else is labelled 0.  Face neighbours of equal value are connected; the blobs of all values together are
    numbered 1 .. n in raster order (C order of the logical index) of their first voxel.
    -> (labels, count) or, with props=True, (labels, count, props): labels int32, contiguous, of the volume's shape, 0 on
    non-members; count int64 [1], the true number of blobs; props int64 [max_blobs, 12], row j - 1 = (value, area, first raster
    index, min0, min1, min2, max0 + 1, max1 + 1, max2 + 1, sum i0, sum i1, sum i2) of blob j: the box is half-open like
    regionprops' bbox and the centroid is sum / area (`region_table` reads it).  Rows from count on are zero; with count >
    max_blobs the labels and count are still complete and props holds the first max_blobs blobs.  max_blobs: 1 .. 2^20,
    ValueError otherwise (and for any other num_classes) before a launch.  An empty volume gives empty labels, count 0 and
    all-zero props.
    HIP tensor: `aide_label_components3d`, seven launches, asynchronous, no host read, HIP tensors returned.  numpy array or CPU
    tensor: scipy.ndimage.label once per value, numpy arrays returned."""
    c = _post_classes(num_classes, 'label_components')
    cap = _max_blobs(max_blobs)
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        _lcc_args(volume)
        v = volume.detach()
        if v.dtype != torch.int64:
            v = v.to(torch.int64)
        labels = torch.empty(v.shape, device=v.device, dtype=torch.int32)
        count = torch.empty(1, device=v.device, dtype=torch.int64)
        table = torch.empty(cap, 12, device=v.device, dtype=torch.int64) if props else None
        ws = torch.empty(lib.aide_label_components3d_ws_bytes(v.numel()), device=v.device, dtype=torch.uint8)
        check(lib.aide_label_components3d(ptr(v), *v.shape, *v.stride(), c or 0, ptr(labels), ptr(count), ptr(table), cap,
                                          ptr(ws), stream_ptr()), 'label_components3d')
        return (labels, count, table) if props else (labels, count)
    vol = _host_volume(volume, 'label_components')
    labels, value, area, first = _label_host(vol, c)
    count = np.array([len(value)], np.int64)
    if not props:
        return labels, count
    return labels, count, _props_host(labels, value, area, first, cap)


def region_table(props, count):
    """The host-side accessor of `label_components(..., props=True)`: one copy to the host, then a dict of numpy arrays over
    the k = min(count, max_blobs) blobs the table holds: count (the true number of blobs, an int), value, area, first (int64
    [k]), bbox (int64 [k, 6]: min0, min1, min2, max0 + 1, max1 + 1, max2 + 1, regionprops' order) and centroid (float64
    [k, 3] = the coordinate sums / area)."""
    if isinstance(props, torch.Tensor) or isinstance(count, torch.Tensor):
        props = torch.as_tensor(props)
        count = torch.as_tensor(count, device=props.device)
        if props.dim() != 2 or props.shape[1] != 12 or count.numel() != 1:
            raise TypeError('region_table: the props [max_blobs, 12] and the count [1] of label_components are expected')
        both = torch.cat([count.reshape(1).to(torch.int64), props.reshape(-1).to(torch.int64)]).cpu().numpy()
    else:
        props, count = np.asarray(props), np.asarray(count)
        if props.ndim != 2 or props.shape[1] != 12 or count.size != 1:
            raise TypeError('region_table: the props [max_blobs, 12] and the count [1] of label_components are expected')
        both = np.concatenate([count.reshape(1).astype(np.int64), props.reshape(-1).astype(np.int64)])
    n, table = int(both[0]), both[1:].reshape(-1, 12)
    table = table[:min(n, len(table))]
    return dict(count=n, value=table[:, 0].copy(), area=table[:, 1].copy(), first=table[:, 2].copy(), bbox=table[:, 3:9].copy(),
                centroid=table[:, 9:12].astype(np.float64) / table[:, 1:2].astype(np.float64))


def _lesion_counts_host(pred, target, c, overlap):
    """the host statement of aide_lesion_counts3d"""
    out = np.zeros((c or 2, 6), np.int64)
    for side, (a, b) in enumerate(((target, pred), (pred, target))):
        labels, value, area, _ = _label_host(a, c)
        agree = (labels > 0) & ((b == a) if c else (b != 0))
        cover = np.bincount(labels[agree].astype(np.int64) - 1, minlength=len(value)).astype(np.int64)
        counts = (cover >= 1) & (cover.astype(np.float64) >= overlap * area.astype(np.float64))
        rows = value if c else np.ones(len(value), np.int64)
        np.add.at(out[:, 2 * side], rows, 1)
        np.add.at(out[:, 2 * side + 1], rows, counts.astype(np.int64))
        if side == 0:
            np.add.at(out[:, 4], rows, cover)
        else:
            np.add.at(out[:, 5], rows, np.where(counts, 0, area))
    return out


def lesion_counts(pred, target, num_classes=None, overlap=0.0):
    """The table behind `lesion_scores`: int64 [rows, 6], rows = num_classes, or 2 with num_classes=None where row 1 is used;
    row 0 is zeros.  Columns: target blobs, target blobs that count, pred blobs, pred blobs that count, the sum of cover over the
    target blobs (the voxel-wise TP of the class), pred voxels in blobs that do not count.  A HIP tensor on either side:
    `aide_lesion_counts3d` (ten launches, no host read), a HIP tensor returned; otherwise the host statement, a numpy array."""
    c = _post_classes(num_classes, 'lesion_scores')
    overlap = _overlap(overlap)
    dev = [x for x in (pred, target) if isinstance(x, torch.Tensor) and x.is_cuda]
    if dev:
        p, t = (torch.as_tensor(x, device=dev[0].device).detach() for x in (pred, target))
        _lcc_args(p)
        _lcc_args(t)
        if tuple(p.shape) != tuple(t.shape):
            raise RuntimeError('lesion_scores: shape mismatch %s vs %s' % (tuple(p.shape), tuple(t.shape)))
        p, t = (x if x.dtype == torch.int64 else x.to(torch.int64) for x in (p, t))
        out = torch.empty(c or 2, 6, device=p.device, dtype=torch.int64)
        ws = torch.empty(lib.aide_lesion_counts3d_ws_bytes(p.numel()), device=p.device, dtype=torch.uint8)
        check(lib.aide_lesion_counts3d(ptr(p), *p.stride(), ptr(t), *t.stride(), *p.shape, c or 0, overlap, ptr(out), ptr(ws),
                                       stream_ptr()), 'lesion_counts3d')
        return out
    p, t = _host_volume(pred, 'lesion_scores'), _host_volume(target, 'lesion_scores')
    if p.shape != t.shape:
        raise RuntimeError('lesion_scores: shape mismatch %s vs %s' % (p.shape, t.shape))
    return _lesion_counts_host(p, t, c, overlap)


def lesion_scores(pred, target, num_classes=None, overlap=0.0):
    """Lesion-wise detection scores of a predicted label volume against its target.  Both volumes (3-D, the same shape, any
    integer dtype and strides) are split into blobs by the rule of `label_components`.  For a blob b of one volume, cover(b) is
    the number of voxels of b at which the other volume agrees: its voxel is not 0 (num_classes=None), or equals b's value
    (num_classes=C).  b counts if and only if cover(b) >= 1 and float64(cover(b)) >= overlap * float64(area(b)); overlap is a
    number in [0, 1] (ValueError otherwise) and the rule is the same on both sides, so swapping the arguments swaps the columns.
    -> dict: the int64 counts target_blobs, detected (target blobs that count), pred_blobs, matched (pred blobs that count),
    covered_voxels (the sum of cover over the target blobs: the voxel-wise TP), spurious_voxels (pred voxels in blobs that do
    not count), and float64 sensitivity = detected / target_blobs, precision = matched / pred_blobs, F1 = 2 S P / (S + P) as
    numpy true divisions (0/0 -> nan, like `case_scores`).  Scalars with num_classes=None, arrays of [C] with num_classes=C
    (entry 0: zeros and nan).  HIP tensors: `aide_lesion_counts3d` and one copy of the table; anything else: the host statement
    through scipy.ndimage.label."""
    table = lesion_counts(pred, target, num_classes, overlap)
    if isinstance(table, torch.Tensor):
        table = table.cpu().numpy()
    rows = table if num_classes is not None else table[1]
    res = {name: (rows[:, k].copy() if num_classes is not None else int(rows[k])) for k, name in enumerate(LESION_COLUMNS)}
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.asarray(rows, np.float64)
        s, p = f[..., 1] / f[..., 0], f[..., 3] / f[..., 2]
        res.update(sensitivity=s, precision=p, F1=2 * s * p / (s + p))
    return res


# ---- all cases of an epoch at once (the epoch end of trainchaos_proposed_30cases1labeled.py:429-496) ----------------
def _starts(slice_start, s_total):
    """the host copy of a slice_start table as a list of ints, checked: K + 1 non-decreasing entries from 0 to S_total"""
    st = [int(v) for v in (slice_start.tolist() if hasattr(slice_start, 'tolist') else slice_start)]
    if len(st) < 1 or st[0] != 0 or st[-1] != s_total or any(b < a for a, b in zip(st, st[1:])):
        raise RuntimeError('slice_start must rise from 0 to the slice count %d, got %r' % (s_total, st))
    return st


def keep_largest_batched(labels, slice_start, num_classes=None, stats=False):
    """[S_total,H,W] integer label maps of K concatenated cases + slice_start[K+1] -> uint8 [S_total,H,W]: for every case
    what `keep_largest_connected_components` gives for its [H,W,S_k] volume.  HIP tensors (slice_start an int64 HIP tensor:
    the table is not read on the host): five launches for any K, no synchronisation.  Anything else: the CPU function per case.
    num_classes=C (2 .. 8): per case what `keep_largest_per_class` gives instead (`aide_keep_largest_cc3d_classes_batched`:
    five launches and one memset for any K and C); stats=True then also returns int64 [K, C, 3], the per-case rows."""
    c = None if num_classes is None else _num_classes(num_classes, 'keep_largest_batched')
    if stats and c is None:
        raise TypeError('keep_largest_batched: stats needs num_classes')
    if isinstance(labels, torch.Tensor) and labels.is_cuda:
        if labels.dim() != 3 or labels.dtype not in _INT_DTYPES:
            raise RuntimeError('keep_largest_batched: [S,H,W] integer labels expected')
        if labels.numel() > _MAX_VOX:
            raise RuntimeError('keep_largest_batched: %d voxels, at most 2^31 - 1' % labels.numel())
        if not (isinstance(slice_start, torch.Tensor) and slice_start.is_cuda and slice_start.dtype == torch.int64
                and slice_start.dim() == 1 and slice_start.numel() >= 1 and slice_start.is_contiguous()):
            raise RuntimeError('keep_largest_batched: slice_start must be a contiguous int64 HIP tensor [K + 1]')
        v = labels.detach().to(torch.int64).contiguous()
        k = slice_start.numel() - 1
        out = torch.empty(v.shape, device=v.device, dtype=torch.uint8)
        if c is not None:
            st = torch.empty(k, c, 3, device=v.device, dtype=torch.int64) if stats else None
            if v.numel() == 0 or k == 0:
                return (out.zero_(), st.zero_()) if stats else out.zero_()
            ws = torch.empty(lib.aide_lcc3d_classes_batched_ws_bytes(v.numel(), k, c), device=v.device, dtype=torch.uint8)
            check(lib.aide_keep_largest_cc3d_classes_batched(ptr(v), ptr(slice_start), k, *v.shape, c, ptr(out), ptr(st),
                                                             ptr(ws), stream_ptr()), 'keep_largest_cc3d_classes_batched')
            return (out, st) if stats else out
        if v.numel() == 0 or k == 0:
            return out.zero_()
        ws = torch.empty(lib.aide_lcc3d_batched_ws_bytes(v.numel(), k), device=v.device, dtype=torch.uint8)
        check(lib.aide_keep_largest_cc3d_batched(ptr(v), ptr(slice_start), k, *v.shape, ptr(out), ptr(ws), stream_ptr()),
              'keep_largest_cc3d_batched')
        return out
    lab = np.asarray(labels)
    st = _starts(slice_start, lab.shape[0])
    out = np.zeros(lab.shape, np.uint8)
    if c is not None:
        rows = np.zeros((len(st) - 1, c, 3), np.int64)
        for k, (a, b) in enumerate(zip(st, st[1:])):
            if b > a:
                keep, rows[k] = _keep_largest_classes_host(lab[a:b].transpose(1, 2, 0), c)
                out[a:b] = keep.transpose(2, 0, 1)
        return (out, rows) if stats else out
    for a, b in zip(st, st[1:]):
        if b > a:
            out[a:b] = keep_largest_connected_components(lab[a:b].transpose(1, 2, 0)).transpose(2, 0, 1)
    return out


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
