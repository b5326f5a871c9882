"""Binary segmentation metrics of utils/metrics2d.py:8-84 on device: one pass of the fused statistics kernel gives, per
image, the hard-prediction count (softmax p1 >= 0.5), the target count and their intersection; every metric below is a
handful of scalar operations on those three numbers.  Results stay on the device (no host sync) unless the reference
itself returns Python numbers (Dice_fn_Nozero)."""
import numpy as np
import torch

from . import _seg
from .._lib import lib, check
from ..ops import ptr, stream_ptr


def _counts(inputs, targets, threshold):
    if threshold != 0.5:
        raise NotImplementedError('aide_amd metrics implement the reference default threshold 0.5')
    with torch.no_grad():
        _, extra = _seg.seg_loss(inputs.detach(), targets, None, 255, 2, 1.0, 1.0, 1.0)
    st = extra['stats']
    hw = float(inputs.shape[2] * inputs.shape[3])
    return extra, st[:, _seg.S_HP], st[:, _seg.S_T], st[:, _seg.S_HI], hw


def Dice_fn(inputs, targets, threshold=0.5):
    """metrics2d.py:8-29: hard Dice summed over the batch (empty target: 1 if the prediction is empty too, else 0)."""
    extra, _, _, _, _ = _counts(inputs, targets, threshold)
    return extra['hard_dice']


def Dice_fn_Nozero(inputs, targets, threshold=0.5):
    """metrics2d.py:31-52: (Dice sum as a Python float, number of images that are not empty in both target and
    prediction).  Syncs, like the reference's .item()."""
    extra, p, t, _, _ = _counts(inputs, targets, threshold)
    count = int(((t != 0) | (p != 0)).sum().item())
    return extra['hard_dice'].item(), count


def TP_TN_FP_FN(inputs, targets, threshold=0.5):
    """metrics2d.py:54-70: confusion counts of the LAST image of the batch (the reference's loop overwrites them per
    image), as 0-dim float tensors."""
    _, p, t, i, hw = _counts(inputs, targets, threshold)
    tp, fp, fn = i[-1], p[-1] - i[-1], t[-1] - i[-1]
    tn = hw - p[-1] - t[-1] + i[-1]
    return tp.float(), tn.float(), fp.float(), fn.float()


def IoU_fn(inputs, targets, threshold=0.5):
    """metrics2d.py:72-84: sum over the batch of |P & T| / |P | T| (NaN for an image empty in both, as the reference)."""
    _, p, t, i, _ = _counts(inputs, targets, threshold)
    return (i.float() / (p + t - i).float()).sum()


# ---- multi-class metrics (metrics2d.py:86-205) -----------------------------------------------------------------------
# The reference copies the logits to the host, takes torch.argmax on the RAW logits (:89) and counts with numpy.  All four
# functions are functions of counts[N][C][3] = (sum i*t, sum i, sum t) per image and class (i, t: one-hot of prediction and
# target).  HIP tensors: one counts launch (csrc/metrics_mc.hip) and ONE copy of N*C*3 int64; anything else: the same counts
# with numpy.  The float64 arithmetic after that is the reference's, operation for operation, so the results have its bits.
_SPECIAL_MODE = 'train3_multidomainl_normalcl'
_MC_MIN, _MC_MAX = 2, 8
_T_ONEHOT_F32, _T_ONEHOT_I64, _T_ONEHOT_U8, _T_INDEX_I64 = 0, 1, 2, 3
ACC_WORDS = 42                  # the accumulator of aide_mc_metrics_accumulate (include/aide_hip.h): 8-byte words


def one_hot_result(label, label_values=((0,), (1,), (2,), (3,), (4,))):
    """metrics2d.py:198-205: [N,K,H,W] labels -> bool [N,len(label_values),H,W], plane j true where all K label channels
    equal label_values[j]."""
    label = np.asarray(label)
    return np.stack([np.all(np.equal(label, value), axis=1) for value in label_values], axis=1)


def _is_dev(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _mc_check(inputs, targets):
    """-> (N, C, H, W, index targets?) after the argument checks; nothing is launched before they pass"""
    ish, tsh = tuple(inputs.shape), tuple(targets.shape)
    if len(ish) != 4:
        raise RuntimeError('multi-class metrics: [N,C,H,W] logits expected, got shape %s' % (ish,))
    n, c, h, w = ish
    if not _MC_MIN <= c <= _MC_MAX:
        raise RuntimeError('multi-class metrics: %d classes, %d .. %d are supported' % (c, _MC_MIN, _MC_MAX))
    dt = inputs.dtype
    if dt not in (torch.float32, np.dtype(np.float32)):
        raise RuntimeError('multi-class metrics: fp32 logits expected, got %s' % (dt,))
    if len(tsh) == 4 and tsh == ish:
        index = False
    elif len(tsh) == 3 and tsh == (n, h, w):
        tdt = targets.dtype
        floating = tdt.is_floating_point if isinstance(tdt, torch.dtype) else np.issubdtype(tdt, np.floating)
        if floating:
            raise RuntimeError('multi-class metrics: [N,H,W] targets are class indices and must be integers, got %s' % (tdt,))
        index = True
    else:
        raise RuntimeError('multi-class metrics: shape mismatch: logits %s, targets %s (one-hot [N,C,H,W] or index [N,H,W])'
                           % (ish, tsh))
    if n > 65535 or c * h * w >= 2 ** 31:
        raise RuntimeError('multi-class metrics: at most 65535 images of C*H*W < 2^31 per call')
    return n, c, h, w, index


def _dense_images(x, inner):
    """x with every image dense (`inner` contiguous elements), any batch stride"""
    if x.shape[0] > 1 and x.stride(0) < inner:
        return x.contiguous()
    return x if x[0].is_contiguous() else x.contiguous()


def _counts_device(inputs, targets):
    n, c, h, w, index = _mc_check(inputs, targets)
    dev = inputs.device
    lg = _dense_images(inputs.detach(), c * h * w)
    tg = targets.detach()
    if tg.device != dev:
        tg = tg.to(dev)
    if index:
        kind = _T_INDEX_I64
        if tg.dtype != torch.int64:
            tg = tg.to(torch.int64)
    elif tg.dtype == torch.float32:
        kind = _T_ONEHOT_F32
    elif tg.dtype == torch.int64:
        kind = _T_ONEHOT_I64
    elif tg.dtype == torch.uint8:
        kind = _T_ONEHOT_U8
    else:
        kind, tg = _T_ONEHOT_U8, (tg != 0).to(torch.uint8)
    tg = _dense_images(tg, h * w if index else c * h * w)
    counts = torch.empty(n, c, 3, device=dev, dtype=torch.int64)
    if n:
        check(lib.aide_mc_counts_logits(ptr(lg), lg.stride(0), ptr(tg), kind, tg.stride(0), c, n, h * w, ptr(counts),
                                        stream_ptr()), 'mc_counts_logits')
    return counts


def _counts_host(inputs, targets):
    """the same counts with numpy; the arg-max is torch's own (ties -> lowest class, the first NaN wins)"""
    n, c, h, w, index = _mc_check(inputs, targets)
    lg = inputs.detach() if isinstance(inputs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(inputs))
    pred = torch.argmax(lg, dim=1).numpy().reshape(n, 1, h * w)
    tg = targets.detach().cpu().numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
    classes = np.arange(c).reshape(1, c, 1)
    i = pred == classes
    t = (tg.reshape(n, 1, h * w) == classes) if index else (tg.reshape(n, c, h * w) != 0)
    return np.stack([(i & t).sum(axis=2), i.sum(axis=2), t.sum(axis=2)], axis=2).astype(np.int64)


def multiclass_counts(inputs, targets):
    """counts[N,C,3] int64 = (sum i*t, sum i, sum t) per image and class for [N,C,H,W] fp32 logits (C = 2 .. 8) against
    one-hot [N,C,H,W] targets (0/1-valued: non-zero is read as 1) or class-index [N,H,W] integer targets (an index outside
    [0, C) belongs to no class).  HIP logits: a HIP tensor, one launch, no host synchronisation.  Otherwise a numpy array."""
    if _is_dev(inputs):
        return _counts_device(inputs, targets)
    if _is_dev(targets):
        targets = targets.cpu()
    return _counts_host(inputs, targets)


def _counts_np(inputs, targets):
    cnt = multiclass_counts(inputs, targets)
    hw = int(inputs.shape[2]) * int(inputs.shape[3])
    return (cnt.cpu().numpy() if isinstance(cnt, torch.Tensor) else cnt), hw     # the one device -> host copy


def _dice_images(cnt):
    """[N,C] float64: 2 TP / (sum i + sum t), 1.0 where the union is 0 (:128-132)"""
    inter = (2 * cnt[..., 0]).astype(np.float64)
    union = (cnt[..., 1] + cnt[..., 2]).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        d = inter / union
    d[union == 0] = 1.0
    return d


def _iou_images(cnt):
    """[N,C] float64: TP / (sum i + sum t - TP), 1.0 where the union is 0 (:157-161)"""
    inter = cnt[..., 0].astype(np.float64)
    union = (cnt[..., 1] + cnt[..., 2]).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        v = inter / (union - inter)
    v[union == 0] = 1.0
    return v


def _sum_images(per_image):
    """the reference's `acc = np.zeros(C); for image: acc += value`: the images are added in index order"""
    acc = np.zeros(per_image.shape[1])
    for row in per_image:
        acc += row
    return acc


def MulticlassDice_fn(inputs, targets, mode='eval'):
    """metrics2d.py:111-138: per-class Dice of the arg-max prediction, the mean over the batch as float64 [C].  A mode
    containing 'train3_multidomainl_normalcl': the scalar dice[1:].sum() / (C - 1) of the batch SUM (not divided by N, as
    the reference has it)."""
    cnt, _ = _counts_np(inputs, targets)
    n, c = cnt.shape[:2]
    dice = _sum_images(_dice_images(cnt))
    if _SPECIAL_MODE in mode:
        return dice[1:].sum() / (c - 1)
    return dice / float(n)


def MulticlassIoU_fn(inputs, targets, mode='eval'):
    """metrics2d.py:140-167: per-class IoU, the mean over the batch as float64 [C]; in the special mode the scalar
    iou.sum() / N / C."""
    cnt, _ = _counts_np(inputs, targets)
    n, c = cnt.shape[:2]
    iou = _sum_images(_iou_images(cnt))
    if _SPECIAL_MODE in mode:
        return iou.sum() / float(n) / c
    return iou / float(n)


def _confusion_images(cnt, hw):
    tp, si, st = (cnt[..., k].astype(np.float64) for k in range(3))
    return tp, float(hw) - si - st + tp, si - tp, st - tp


def MulticlassTP_TN_FP_FN(inputs, targets, mode='eval'):
    """metrics2d.py:169-196: (TP, TN, FP, FN), each float64 [C]: the sums over the batch divided by N (every mode)."""
    cnt, hw = _counts_np(inputs, targets)
    n = cnt.shape[0]
    return tuple(_sum_images(v) / float(n) for v in _confusion_images(cnt, hw))


def MulticlassAccuracy_fn(inputs, targets, mode='eval'):
    """metrics2d.py:86-109: correctly labelled pixels, summed over the batch and divided by N (special mode: by H, then
    by W), a numpy float64.  The reference hard-codes the five label values 0 .. 4 (:95) and fails with a ValueError for
    every other class count; so does this function, before anything is launched."""
    c = int(inputs.shape[1]) if len(inputs.shape) == 4 else -1
    if c != 5:
        _mc_check(inputs, targets)
        raise ValueError('MulticlassAccuracy_fn is defined for 5 classes only: the reference hard-codes the label values '
                         '0 .. 4 and raises ValueError for C = %d as well' % c)
    cnt, _ = _counts_np(inputs, targets)
    n = cnt.shape[0]
    correct = np.float64(0)
    for row in cnt[..., 0]:
        correct = correct + np.float64(row.sum())
    if _SPECIAL_MODE in mode:
        return correct / float(inputs.shape[2]) / float(inputs.shape[3])
    return correct / float(n)


class MulticlassMeter(object):
    """Running multi-class metrics of an epoch without a per-batch host read.

    update(inputs, targets): the counts launch and one launch that adds the batch to a 42-word device accumulator
    (include/aide_hip.h, aide_mc_metrics_accumulate); returns nothing.  compute(): the one copy of the epoch -> dict of
    `dice`, `iou` (float64 [C]: the means over all images seen, under MulticlassDice_fn's / MulticlassIoU_fn's rules, added in
    the order the images came), `TP`, `TN`, `FP`, `FN` (float64 [C]: the means per image, as MulticlassTP_TN_FP_FN) and
    `images`.  On a non-HIP device the same sums are kept with numpy."""

    def __init__(self, num_classes, device):
        if not _MC_MIN <= int(num_classes) <= _MC_MAX:
            raise RuntimeError('MulticlassMeter: %d classes, %d .. %d are supported' % (num_classes, _MC_MIN, _MC_MAX))
        self.num_classes = int(num_classes)
        self.device = torch.device(device)
        self.reset()

    def reset(self):
        if self.device.type == 'cuda':
            self._acc = torch.zeros(ACC_WORDS, device=self.device, dtype=torch.int64)
        else:
            self._acc = np.zeros(ACC_WORDS, np.int64)

    def update(self, inputs, targets):
        c = self.num_classes
        if len(inputs.shape) != 4 or inputs.shape[1] != c:
            raise RuntimeError('MulticlassMeter(%d): logits of shape %s' % (c, tuple(inputs.shape)))
        n, hw = int(inputs.shape[0]), int(inputs.shape[2]) * int(inputs.shape[3])
        if self.device.type == 'cuda':
            if not _is_dev(inputs) or inputs.device != self.device:
                raise RuntimeError('MulticlassMeter on %s: logits on %s' % (self.device, getattr(inputs, 'device', 'the host')))
            cnt = _counts_device(inputs, targets)
            if n:
                check(lib.aide_mc_metrics_accumulate(ptr(cnt), n, c, hw, ptr(self._acc), stream_ptr()), 'mc_metrics_accumulate')
            return
        cnt = multiclass_counts(inputs, targets)
        f = self._acc.view(np.float64)
        for row_d, row_i in zip(_dice_images(cnt), _iou_images(cnt)):
            f[0:c] += row_d
            f[8:8 + c] += row_i
        for k in range(3):
            self._acc[16 + 8 * k:16 + 8 * k + c] += cnt[..., k].sum(axis=0)
        self._acc[40] += n
        self._acc[41] += n * hw

    def compute(self):
        c = self.num_classes
        acc = self._acc.cpu().numpy() if isinstance(self._acc, torch.Tensor) else self._acc.copy()
        f = acc.view(np.float64)
        images, pixels = int(acc[40]), int(acc[41])
        tp, si, st = (acc[16 + 8 * k:16 + 8 * k + c].astype(np.float64) for k in range(3))
        with np.errstate(divide='ignore', invalid='ignore'):
            n = float(images)
            return dict(dice=f[0:c] / n, iou=f[8:8 + c] / n, TP=tp / n, TN=(float(pixels) - si - st + tp) / n,
                        FP=(si - tp) / n, FN=(st - tp) / n, images=images)
