"""Post-processing of a predicted label volume and lesion-wise detection, on the device with scipy statements on the host:
the largest-component filters, the k largest blobs with a size floor, hole filling, labelled components with their region
table, and the lesion counts and scores (aide_amd/csrc/eval3d.hip).  `aide_amd.inference` re-exports
every name."""
import numpy as np
import torch

from ._lib import lib, check
from .ops import ptr, stream_ptr
from .volumes import INT_DTYPES, MAX_VOX, classes, device_volume, host_volume, u8, volume_args, widen, workspace


def keep_largest_connected_components(mask):
    """trainchaos_comparison_1case.py:68-77 / trainchaos_proposed_30cases1labeled.py:103-112: the largest connected blob of a
    label volume (connectivity 1: face neighbours), uint8.  CPU post-processing in the reference (skimage.measure.label +
    regionprops).  skimage connects neighbours of EQUAL value (0 = background) and numbers the blobs in raster order of
    their first voxel; scipy.ndimage.label connects every non-zero voxel, so it is run once per label value and the blobs
    are ordered by their first voxel -- the same blob as the reference's `np.argmax(area)` on ties, and for a multi-class
    volume (num_classes up to 8 here) blobs of different classes stay separate as they do there."""
    if isinstance(mask, torch.Tensor) and mask.is_cuda:
        return _keep_largest_device(mask)
    mask = np.asarray(mask)
    out = np.zeros(mask.shape, dtype=np.uint8)
    if mask.size == 0 or mask.max() <= 0:
        return out
    best = None                                   # ((area, -first voxel), blob labels, blob id)
    for v in np.unique(mask):
        if v == 0:
            continue
        blobs, area, first = _blobs_of(mask, v)
        for b in range(len(area)):
            cand = (int(area[b]), -int(first[b]))
            if best is None or cand > best[0]:
                best = (cand, blobs, b + 1)
    out[best[1] == best[2]] = 1
    return out


def _keep_largest_device(mask):
    """HIP tensor (d0, d1, d2) of integer labels, any strides -> uint8 HIP tensor of the same shape (1 on the largest
    blob); raster order is C order of the LOGICAL index.  Asynchronous: no host synchronisation."""
    mask = device_volume(mask, 'keep_largest_connected_components')
    out = torch.empty(mask.shape, device=mask.device, dtype=torch.uint8)
    if mask.numel() == 0:
        return out
    ws = workspace(lib.aide_lcc3d_ws_bytes, mask)
    check(lib.aide_keep_largest_cc3d(ptr(mask), *mask.shape, *mask.stride(), ptr(out), ptr(ws), stream_ptr()),
          'keep_largest_cc3d')
    return out


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
    c = classes(num_classes, 'keep_largest_per_class', strict=False)
    if isinstance(mask, torch.Tensor) and mask.is_cuda:
        out, st = _keep_largest_classes_device(mask, c, stats)
    else:
        if isinstance(mask, torch.Tensor):
            mask = mask.detach().numpy()
        out, st = _keep_largest_classes_host(np.asarray(mask), c)
    return (out, st) if stats else out


def _keep_largest_classes_host(mask, c):
    out = np.zeros(mask.shape, dtype=np.uint8)
    st = np.zeros((c, 3), dtype=np.int64)
    if mask.size == 0:
        return out, st
    for v in range(1, c):
        blobs, area, first = _blobs_of(mask, v)
        if len(area) == 0:
            continue
        b = max(range(len(area)), key=lambda j: (int(area[j]), -int(first[j])))
        out[blobs == b + 1] = v
        st[v] = len(area), int(area.sum()), int(area[b])
    return out, st


def _keep_largest_classes_device(mask, c, stats):
    mask = device_volume(mask, 'keep_largest_per_class')
    out = torch.empty(mask.shape, device=mask.device, dtype=torch.uint8)
    st = torch.empty(c, 3, device=mask.device, dtype=torch.int64) if stats else None
    if mask.numel() == 0:
        return out, (st.zero_() if stats else None)
    ws = workspace(lib.aide_lcc3d_classes_ws_bytes, mask, c)
    check(lib.aide_keep_largest_cc3d_classes(ptr(mask), *mask.shape, *mask.stride(), c, ptr(out), ptr(st), ptr(ws),
                                             stream_ptr()), 'keep_largest_cc3d_classes')
    return out, st


# ---- case post-processing: the k largest blobs with a size floor, hole filling ------------------------------------------
MAX_TOP_K = 8


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
    c = classes(num_classes, 'keep_components')
    if stats and c is None:
        raise TypeError('keep_components: stats needs num_classes')
    ks = _per_class(top_k, c, 'top_k', _top_k)
    ms = _per_class(min_voxels, c, 'min_voxels', _min_voxels)
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        import ctypes
        v = device_volume(volume, 'keep_components')
        out = torch.empty(v.shape, device=v.device, dtype=torch.uint8)
        st = torch.empty(c, 3, device=v.device, dtype=torch.int64) if stats else None
        if v.numel() == 0:
            return (out, st.zero_()) if stats else out
        ws = workspace(lib.aide_components3d_ws_bytes, v)
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
    c = classes(num_classes, 'fill_holes')
    if slice_axis is not None and (isinstance(slice_axis, bool) or not isinstance(slice_axis, (int, np.integer))
                                   or not 0 <= slice_axis <= 2):
        raise ValueError('fill_holes: slice_axis %r, None, 0, 1 or 2 are supported' % (slice_axis,))
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        v = device_volume(volume, 'fill_holes', keep_uint8=True)
        out = torch.empty(v.shape, device=v.device, dtype=torch.uint8)
        st = torch.empty(c or 2, 2, device=v.device, dtype=torch.int64) if stats else None
        if v.numel() == 0:
            return (out, st.zero_()) if stats else out
        ws = workspace(lib.aide_fill_holes3d_ws_bytes, v)
        check(lib.aide_fill_holes3d(ptr(v), u8(v), *v.shape, *v.stride(), c or 0,
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
    c = classes(num_classes, 'label_components')
    cap = _max_blobs(max_blobs)
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        v = device_volume(volume, 'label_components')
        labels = torch.empty(v.shape, device=v.device, dtype=torch.int32)
        count = torch.empty(1, device=v.device, dtype=torch.int64)
        table = torch.empty(cap, 12, device=v.device, dtype=torch.int64) if props else None
        ws = workspace(lib.aide_label_components3d_ws_bytes, v)
        check(lib.aide_label_components3d(ptr(v), *v.shape, *v.stride(), c or 0, ptr(labels), ptr(count), ptr(table), cap,
                                          ptr(ws), stream_ptr()), 'label_components3d')
        return (labels, count, table) if props else (labels, count)
    vol = host_volume(volume, 'label_components')
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
    c = classes(num_classes, 'lesion_scores')
    overlap = _overlap(overlap)
    dev = [x for x in (pred, target) if isinstance(x, torch.Tensor) and x.is_cuda]
    if dev:
        p, t = (torch.as_tensor(x, device=dev[0].device) for x in (pred, target))
        volume_args(p, 'lesion_scores')
        volume_args(t, 'lesion_scores')
        if tuple(p.shape) != tuple(t.shape):
            raise RuntimeError('lesion_scores: shape mismatch %s vs %s' % (tuple(p.shape), tuple(t.shape)))
        p, t = widen(p), widen(t)
        out = torch.empty(c or 2, 6, device=p.device, dtype=torch.int64)
        ws = workspace(lib.aide_lesion_counts3d_ws_bytes, p)
        check(lib.aide_lesion_counts3d(ptr(p), *p.stride(), ptr(t), *t.stride(), *p.shape, c or 0, overlap, ptr(out), ptr(ws),
                                       stream_ptr()), 'lesion_counts3d')
        return out
    p, t = host_volume(pred, 'lesion_scores'), host_volume(target, 'lesion_scores')
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
    c = None if num_classes is None else classes(num_classes, 'keep_largest_batched', strict=False)
    if stats and c is None:
        raise TypeError('keep_largest_batched: stats needs num_classes')
    if isinstance(labels, torch.Tensor) and labels.is_cuda:
        if labels.dim() != 3 or labels.dtype not in INT_DTYPES:
            raise RuntimeError('keep_largest_batched: [S,H,W] integer labels expected')
        if labels.numel() > MAX_VOX:
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
            ws = workspace(lib.aide_lcc3d_classes_batched_ws_bytes, v, k, c)
            check(lib.aide_keep_largest_cc3d_classes_batched(ptr(v), ptr(slice_start), k, *v.shape, c, ptr(out), ptr(st),
                                                             ptr(ws), stream_ptr()), 'keep_largest_cc3d_classes_batched')
            return (out, st) if stats else out
        if v.numel() == 0 or k == 0:
            return out.zero_()
        ws = workspace(lib.aide_lcc3d_batched_ws_bytes, v, k)
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
