"""The proposed loaders' transform chain on the GPU, for a whole batch (aide_amd/csrc/augment.hip).

The reference builds the four augmented views of every sample in its DataLoader workers with PIL
(datasetchaos_proposed/transform.py: Resize(BILINEAR) -> RandomRotate(BILINEAR) -> RandomHorizontallyFlip -> ToTensor ->
Normalize, and the single-modal copies of datasetkidney_proposed/, datasetprostate_proposed/, datasetbreast_proposed/).
LoaderAugment takes the decoded slices (grey u8, or raw u16 as pydicom yields them) and returns what that Compose + the
default collate return, as device tensors: the base images, the `augset` dict and the one-hot masks of dataset.py.  The u8
stages (resize, rotation, flip) are bit-exact with PIL; ToTensor + Normalize is float32 as torch does it, with the per-image
mean / std formed from exact integer sums.

The host builds small index / weight tables (PIL's resampling coefficients, cached per size pair) and uploads them with the
packed source planes and the rotation parameters in ONE pinned copy; the device work is two launches (three with masks),
all on the current stream, with no host synchronisation."""
import functools
import math

import numpy as np
import torch

from .._lib import lib, check
from ..ops import stream_ptr
from .augment import pil_rotate_params, _aug_rows

CHAOS_PALETTE = (0, 63, 126, 189, 252)       # datasetchaos_proposed/dataset.py: palette = [[0], [63], [126], [189], [252]]
_PREC = 22                                    # Resample.c PRECISION_BITS (8-bit images)


def draw_aug_params(n, rotation, rng, augno=4):
    """The random draws of the reference's RandomRotate + RandomHorizontallyFlip for n samples, in its order: per sample
    `augno` angles (random.random() * 2 * degree - degree), then `augno` flips (random.random() < 0.5).  rng: a Python
    random.Random (or the `random` module) -- seeded as the loader's worker, it draws what the reference loader draws.
    -> {'augno': [augno] * n, 'degree{k}': [n floats], 'hflip{k}': [n ints]}, the collated bookkeeping of dataset.py."""
    if not 0 <= augno <= 4:
        raise ValueError('augno must be in 0..4')
    out = {'augno': [augno] * n}
    for k in range(augno):
        out['degree%d' % (k + 1)] = []
        out['hflip%d' % (k + 1)] = []
    for _ in range(n):
        for k in range(augno):
            out['degree%d' % (k + 1)].append(rng.random() * 2 * rotation - rotation)
        for k in range(augno):
            out['hflip%d' % (k + 1)].append(1 if rng.random() < 0.5 else 0)
    return out


@functools.lru_cache(maxsize=64)
def bilinear_table(in_size, out_size):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc (Resample.c) for the triangle filter, one row per output index:
    [first tap, taps, k weights (22-bit fixed point, 0 past `taps`)] -> (int32 [out, k + 2], k)"""
    scale = float(in_size) / out_size
    fs = max(scale, 1.0)
    support = fs
    k = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    taps = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    ss = 1.0 / fs
    w = np.zeros((out_size, k))
    for x in range(k):
        t = np.abs(((x + xmin) - center + 0.5) * ss)
        w[:, x] = np.where(x < taps, np.where(t < 1.0, 1.0 - t, 0.0), 0.0)
    ww = np.zeros(out_size)
    for x in range(k):                        # (summed in tap order, as the C loop does)
        ww = ww + w[:, x]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.where(w < 0, (-0.5 + w * (1 << _PREC)).astype(np.int64), (0.5 + w * (1 << _PREC)).astype(np.int64))
    return np.concatenate([xmin[:, None], taps[:, None], kk], axis=1).astype(np.int32), k


@functools.lru_cache(maxsize=64)
def nearest_index(in_size, out_size):
    """Source index per output index of PIL's resize(NEAREST): ImagingScaleAffine accumulates the scale (xo = s / 2, then
    xo += s per step), which is not always int((i + 0.5) * in / out)."""
    s = float(in_size) / out_size
    steps = np.full(out_size, s)
    steps[0] = s * 0.5
    return np.minimum(np.add.accumulate(steps).astype(np.int64), in_size - 1).astype(np.int32)


def resize_bilinear_model(a, size):
    """numpy model of the device resize (PIL Image.resize(BILINEAR) of a grey / clamped-u16 plane) on the same tables"""
    a = np.minimum(np.asarray(a).astype(np.int64), 255)
    h, w = a.shape
    def clip8(v):
        return np.where(v >= 1 << 30, 255, np.where(v <= 0, 0, v >> _PREC))
    def one(a, n_in, tab, k, axis):
        acc = np.full(a.shape[:axis] + (tab.shape[0],) + a.shape[axis + 1:], 1 << (_PREC - 1), np.int64)
        for t in range(k):
            idx = np.minimum(tab[:, 0] + t, n_in - 1)
            wt = np.where(t < tab[:, 1], tab[:, 2 + t], 0).astype(np.int64)
            acc += np.take(a, idx, axis=axis) * (wt if axis == 1 else wt[:, None])
        return clip8(acc)
    tx, kx = bilinear_table(w, size)
    ty, ky = bilinear_table(h, size)
    return one(one(a, w, tx, kx, 1), h, ty, ky, 0).astype(np.uint8)


def _as_planes(sample):
    return list(sample) if isinstance(sample, (tuple, list)) else [sample]


class _Packer(object):
    """one host buffer: 16-byte aligned regions, addressed by byte offset"""

    def __init__(self):
        self.parts, self.size = [], 0

    def add(self, arr):
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        off = self.size
        self.parts.append((off, b))
        self.size = (off + b.size + 15) & ~15
        return off

    def fill(self, buf):
        for off, b in self.parts:
            buf[off:off + b.size] = b
        return buf

    def host(self):
        return self.fill(np.zeros(max(self.size, 16), np.uint8))

    def upload(self, device):
        host = torch.empty(max(self.size, 16), dtype=torch.uint8).pin_memory()
        self.fill(host.numpy())
        return host.to(device, non_blocking=True)


class LoaderAugment(object):
    """Callable form of the proposed loaders' Compose + collate on the device.

    LoaderAugment(img_size, rotation, data_mean=None, data_std=None, palette=CHAOS_PALETTE)(images, params, masks=None)
      images: N samples, each a 2-D u8 / u16 array (single-modal) or a tuple of M of them (two-modal: in-phase, out-phase);
              samples may differ in size
      params: draw_aug_params(N, rotation, rng) (its 'augno', 'degree{k}', 'hflip{k}')
      masks:  None, or N samples of a 2-D u8 mask or a tuple of Q of them (dataset.py's mask, mask1, mask2)
    -> (base, augset, onehot): base = M tensors [N,3,S,S] (the Resize'd, normalised images), augset = params plus the
       views 'imgmodal{m}{k}' (M = 2) or 'img{k}' (M = 1), each [N,3,S,S]; onehot = Q int64 tensors [N,len(palette),S,S].
    raw=True returns the u8 stages instead: base M x [N,S,S], the views [N,S,S] (one channel of the RGB image).
    rotation is the RandomRotate degree range (what draw_aug_params draws from); the call itself uses the drawn angles."""

    def __init__(self, img_size, rotation, data_mean=None, data_std=None, palette=CHAOS_PALETTE):
        self.size = int(img_size)
        self.rotation = float(rotation)
        if (data_mean is None) != (data_std is None):
            raise ValueError('data_mean and data_std go together')
        self.norm = None
        if data_mean is not None:
            mean, std = np.asarray(data_mean, np.float32), np.asarray(data_std, np.float32)
            self.norm = np.concatenate([np.broadcast_to(mean, (3,)), np.broadcast_to(std, (3,))]).astype(np.float32)
        self.palette = np.asarray(palette, np.int32)
        if not 1 <= self.palette.size <= 8:
            raise ValueError('palette: 1 to 8 values')

    def pack(self, images, params, masks=None):
        """host side of a call: the one buffer that is uploaded (source planes, PIL tables, descriptors, rotation rows) and
        where its parts lie -> (_Packer, dict of counts and byte offsets).  Descriptor row p = n * M + m describes source plane
        m of sample n; mask row q * N + n describes mask q of sample n."""
        S = self.size
        samples = [_as_planes(s) for s in images]
        N, M = len(samples), len(samples[0]) if samples else 0
        if N == 0 or any(len(s) != M for s in samples):
            raise ValueError('every sample needs the same number of modalities')
        A = int(params['augno'][0]) if len(params['augno']) else 0
        if any(int(a) != A for a in params['augno']) or not 0 <= A <= 4:
            raise ValueError('augno must be one value in 0..4 for the whole batch')
        pk = _Packer()
        tabs, desc, srcs = [], np.zeros((N * M, 8), np.int32), [None] * (N * M)
        ntab = [0]

        def table(arr):
            off = ntab[0]
            tabs.append(arr.reshape(-1))
            ntab[0] += arr.size
            return off
        tab_ids = {}
        for n, planes in enumerate(samples):
            for m, a in enumerate(planes):
                a = np.asarray(a)
                if a.ndim != 2 or a.dtype not in (np.uint8, np.uint16):
                    raise ValueError('source planes are 2-D u8 or u16 arrays, got %s %s' % (a.dtype, a.shape))
                h, w = a.shape
                for d in (w, h):
                    if ('b', d) not in tab_ids:
                        t, k = bilinear_table(d, S)
                        tab_ids[('b', d)] = (table(t), k)
                (xo, kx), (yo, ky) = tab_ids[('b', w)], tab_ids[('b', h)]
                srcs[n * M + m] = a
                desc[n * M + m] = (0, h, w, int(a.dtype == np.uint16), xo, yo, kx, ky)
        mdesc, msrcs, Q = None, [], 0
        if masks is not None:
            msamples = [_as_planes(s) for s in masks]
            Q = len(msamples[0]) if msamples else 0
            if len(msamples) != N or any(len(s) != Q for s in msamples):
                raise ValueError('masks: one entry per sample, the same count each')
            mdesc, msrcs = np.zeros((Q * N, 8), np.int32), [None] * (Q * N)
            for n, planes in enumerate(msamples):
                for q, a in enumerate(planes):
                    a = np.asarray(a)
                    if a.ndim != 2 or a.dtype != np.uint8:
                        raise ValueError('mask planes are 2-D u8 arrays (mode L)')
                    h, w = a.shape
                    for d in (w, h):
                        if ('n', d) not in tab_ids:
                            tab_ids[('n', d)] = (table(nearest_index(d, S)), 0)
                    msrcs[q * N + n] = a            # (row order of the descriptors, not the order of the loops)
                    mdesc[q * N + n] = (0, h, w, 0, tab_ids[('n', w)][0], tab_ids[('n', h)][0], 0, 0)
        # rotation rows of the forward views [N][A][8] and, for reverseaug, of the inverse maps [A][N][8]
        fwd = np.zeros((N, max(A, 1), 8), np.float64)
        rev = []
        for k in range(A):
            flips, degs = params['hflip%d' % (k + 1)], params['degree%d' % (k + 1)]
            for n in range(N):
                mtx, mode = pil_rotate_params(float(degs[n]), S, S)
                fwd[n, k] = mtx + [1.0 if int(flips[n]) else 0.0, float(mode)]
            rev.append(_aug_rows(N, S, S, [int(f) for f in flips], [float(d) for d in degs]))
        o = dict(N=N, M=M, A=A, Q=Q)
        o['par'] = pk.add(fwd)
        o['rev'] = pk.add(np.asarray(rev, np.float64).reshape(max(A, 1) * N * 8) if A else np.zeros(8))
        o['norm'] = pk.add(self.norm) if self.norm is not None else None
        o['pal'] = pk.add(self.palette)
        desc[:, 0] = [pk.add(a) for a in srcs]
        o['desc'] = pk.add(desc)
        o['mdesc'] = None
        if mdesc is not None:
            mdesc[:, 0] = [pk.add(a) for a in msrcs]
            o['mdesc'] = pk.add(mdesc)
        o['tab'] = pk.add(np.concatenate(tabs).astype(np.int32))
        if pk.size >= 1 << 31:
            raise ValueError('batch too large for one upload (2 GiB)')
        return pk, o

    def __call__(self, images, params, masks=None, raw=False, device=None):
        S = self.size
        device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        pk, o = self.pack(images, params, masks)
        N, M, A, Q = o['N'], o['M'], o['A'], o['Q']
        o_desc, o_tab, o_par, o_norm, o_pal, o_mdesc, o_rev = (o['desc'], o['tab'], o['par'], o['norm'], o['pal'], o['mdesc'],
                                                                o['rev'])
        dev = pk.upload(device)
        base_ptr = dev.data_ptr()
        st = stream_ptr()

        out_u8 = 1 if raw else 0
        out = torch.empty((M, A + 1, N) + ((S, S) if raw else (3, S, S)), dtype=torch.uint8 if raw else torch.float32,
                          device=device)
        ws = torch.empty(lib.aide_loader_aug_ws_bytes(N * M, S), dtype=torch.uint8, device=device)
        check(lib.aide_loader_aug(base_ptr, base_ptr + o_desc, base_ptr + o_tab, base_ptr + o_par,
                                  base_ptr + o_norm if o_norm is not None else None, N, M, S, A, out_u8, out.data_ptr(),
                                  ws.data_ptr(), st), 'loader_aug')
        onehot = []
        if Q:
            oh = torch.empty((Q, N, int(self.palette.size), S, S), dtype=torch.int64, device=device)
            check(lib.aide_loader_mask_onehot(base_ptr, base_ptr + o_mdesc, base_ptr + o_tab, base_ptr + o_pal, Q * N, S,
                                              int(self.palette.size), oh.data_ptr(), st), 'loader_mask_onehot')
            onehot = [oh[q] for q in range(Q)]
        augset = {key: list(v) for key, v in params.items()}
        for k in range(A):
            for m in range(M):
                augset[('imgmodal%d%d' % (m + 1, k + 1)) if M > 1 else ('img%d' % (k + 1))] = out[m, k + 1]
        if A:
            # reverseaug's parameter rows for logits of this size, already on the device (no second upload)
            augset['_aide_revpar'] = (dev[o_rev:o_rev + A * N * 64].view(torch.float64).view(A, N, 8), (S, S))
        # (`dev` and `ws` are released to the caching allocator in stream order: the launches above are queued on the current stream)
        return [out[m, 0] for m in range(M)], augset, onehot
