"""Pseudo-label bank: AIDE's label self-correction without the PNG round trip.

Reference (train_files/trainchaos_proposed_30cases1labeled.py:429-496, :528-575): after every epoch both networks predict
every training case, the largest 3-D component of each prediction is scored against the case's CURRENT pseudo-label
(`mask1[1]` / `mask2[1]`: the plane of palette value 63 of `<mask>_net1.png` / `_net2.png`, or of the original mask while no
such file exists, datasetchaos_proposed/dataset.py:37-56), and while `(epoch + 1) <= warmup_epoch or (epoch + 1) % 10 == 0`
the worst quarter of the cases -- the labelled ones excepted -- get `prediction * 63` written as their new PNGs.

Here the PNG bytes live in `bank[2][S_total][H][W]` (uint8, one plane per network, both starting as the initial masks); all
cases are evaluated in one batched pass, the rule runs on the device and the selected cases' slices are rewritten in place
(`aide_keep_largest_cc3d_batched`, `aide_case_confusion_batched`, `aide_label_refresh_select`, `aide_label_bank_update`); the
next epoch's targets are gathered from the bank as the loader's one-hot (`aide_label_bank_targets`).  With numpy / CPU
masks the same integers are computed with numpy (and the scipy filter): the form the tests without a GPU run.

Ranking: ascending Dice, NaN greatest (as torch's sort), equal values by the lower case index.  The last is this
project's rule: the reference's `Tensor.sort()` is not stable, so a tie at the selection boundary has no defined winner
there.

`PseudoLabelBank(..., num_classes=C)` is the multi-organ form (the reference's scripts are liver-only, so the rule is this
project's, `inference.case_dice_rule_classes`): class c <-> palette[c], the case score is the mean Dice of the organs present
in the prediction or the pseudo-label, and the selected cases get `palette[prediction]` (`aide_case_class_counts_batched`,
`aide_label_refresh_select_classes`, `aide_label_bank_update_classes`); `targets(index=True)` gathers class-index targets
(`aide_label_bank_targets_index`).

`ImageLabelBank` is the per-IMAGE form of the kidney and breast scripts (no component filter, Dice2d with union == 0 -> 0.0,
`--update_percent`, an empty prediction is never written; `aide_image_*` of csrc/labelbank.hip): see its docstring."""
import os

import numpy as np
import torch

from .inference import evaluate_label_maps, predict_labels

CHAOS_PALETTE = (0, 63, 126, 189, 252)       # datasetchaos_proposed/dataset.py:9
LIVER = 63                                   # palette[1]: the plane the case Dice is taken against, and prediction * 63


def refresh_gate(epoch, warmup_epoch):
    """:528 -- whether the pseudo-labels are rewritten after (0-based) `epoch`"""
    return (epoch + 1) <= warmup_epoch or (epoch + 1) % 10 == 0


class PseudoLabelBank(object):
    """initial_masks_u8: [S_total,H,W] uint8, the slices of K cases concatenated (palette bytes, what the loader decodes from
    the mask PNG); slice_start: K + 1 ints; labelled_cases: indices of the cases whose labels are never rewritten.
    A HIP tensor (or device=...) keeps the bank on the device; numpy / CPU input keeps a numpy bank.
    num_classes=C (2 .. 8, == len(palette), distinct palette bytes): the multi-organ form -- every case is scored per class
    against the planes `bank byte == palette[c]` and rewritten with `palette[prediction]`; `case_dice()`, `modify_list`,
    `export_png`, the gate and `n_select` keep their rules (the bank bytes are the PNG bytes either way)."""

    def __init__(self, initial_masks_u8, slice_start, labelled_cases, palette=CHAOS_PALETTE, device=None, case_ids=None,
                 num_classes=None):
        on_dev = isinstance(initial_masks_u8, torch.Tensor) and initial_masks_u8.is_cuda
        if device is None and on_dev:
            device = initial_masks_u8.device
        self.device = torch.device(device) if device is not None else None
        if self.device is not None and self.device.type != 'cuda':
            self.device = None
        m = initial_masks_u8
        if m.dtype not in (torch.uint8, np.uint8) or len(m.shape) != 3:
            raise RuntimeError('PseudoLabelBank: [S,H,W] uint8 masks expected')
        self.slice_start = [int(v) for v in slice_start]
        s = self.slice_start
        if len(s) < 1 or s[0] != 0 or s[-1] != m.shape[0] or any(b < a for a, b in zip(s, s[1:])):
            raise RuntimeError('PseudoLabelBank: slice_start must rise from 0 to %d, got %r' % (m.shape[0], s))
        self.K = len(s) - 1
        self.palette = tuple(int(p) for p in palette)
        if not 1 <= len(self.palette) <= 8:
            raise RuntimeError('PseudoLabelBank: 1 .. 8 palette values')
        self.match = self.palette[1] if len(self.palette) > 1 else self.palette[0]
        self.num_classes = None if num_classes is None else int(num_classes)
        if self.num_classes is not None:
            c = self.num_classes
            if not 2 <= c <= 8 or c != len(self.palette) or len(set(self.palette)) != c or \
                    any(not 0 <= v <= 255 for v in self.palette):
                raise ValueError('PseudoLabelBank: num_classes %d needs a palette of as many distinct bytes (2 .. 8), got %r'
                                 % (c, self.palette))
        lab = np.zeros(self.K, np.uint8)
        for k in labelled_cases:
            lab[int(k)] = 1
        self.labelled_host = lab
        self.case_ids = list(case_ids) if case_ids is not None else list(range(self.K))
        self.n_select = int(0.25 * self.K)                       # :529
        if self.device is not None:
            m = torch.as_tensor(m).to(self.device)
            self.bank = torch.stack([m, m]).contiguous()
            self._start = torch.tensor(s, dtype=torch.int64).to(self.device)
            self._labelled = torch.from_numpy(lab).to(self.device)
            self._palette = torch.tensor(self.palette, dtype=torch.int32).to(self.device)
            self._dice = torch.zeros(2, self.K, device=self.device, dtype=torch.float32)
            self._class_dice = torch.zeros(2, self.K, self.num_classes or 0, device=self.device, dtype=torch.float32)
            self.rank = torch.zeros(2, self.K, device=self.device, dtype=torch.int32)
            self.selected = torch.zeros(2, self.K, device=self.device, dtype=torch.uint8)
            self.modified = torch.zeros(2, self.K, device=self.device, dtype=torch.uint8)
        else:
            m = np.ascontiguousarray(m.numpy() if isinstance(m, torch.Tensor) else m)
            self.bank = np.stack([m, m])
            self._dice = np.zeros((2, self.K), np.float32)
            self._class_dice = np.zeros((2, self.K, self.num_classes or 0), np.float32)
            self.rank = np.zeros((2, self.K), np.int32)
            self.selected = np.zeros((2, self.K), np.uint8)
            self.modified = np.zeros((2, self.K), np.uint8)

    # ---- epoch end ----
    def refresh_from_labels(self, labels1, labels2, epoch, warmup_epoch, keep_largest=True):
        """labels1 / labels2: the two networks' label maps [S_total,H,W] of all cases.  Case Dice and ranking are taken every
        epoch; the selected cases' planes are rewritten only while the gate of :528 is open.  -> whether it was.  On the
        device: no host synchronisation (`selected` never leaves it).  With num_classes the label maps carry class values
        0 .. C - 1, the filter is the per-class one, and a selected case gets `palette[filtered]` (a value >= C, which only an
        unfiltered map can hold, writes palette[0])."""
        write = refresh_gate(epoch, warmup_epoch)
        c = self.num_classes
        dev = self.device is not None
        start, labelled, palette = (self._start, self._labelled, self._palette) if dev else \
            (self.slice_start, self.labelled_host, self.palette)
        for n, labels in enumerate((labels1, labels2)):
            if dev and not (isinstance(labels, torch.Tensor) and labels.is_cuda):
                raise RuntimeError('PseudoLabelBank: the bank is on %s, the label maps must be too' % self.device)
            r = evaluate_label_maps(labels if dev else np.asarray(labels), start, self.bank[n], self.match, labelled, self.n_select,
                                    keep_largest, num_classes=c, palette=palette if c else None)
            self._dice[n][...], self.rank[n][...], self.selected[n][...] = r['dice'], r['rank'], r['selected']
            if c:
                self._class_dice[n][...] = r['class_dice']
            if write:
                self._rewrite(self.bank[n], r['filtered'], r['selected'])
                modified = self.modified[n]
                modified |= r['selected']
        return write

    def _rewrite(self, plane, filtered, selected):
        """the selected cases' slices of `plane` = the byte map of `filtered`: `* LIVER` (:549-550), with num_classes
        `palette[v]` and palette[0] for a value >= C.  On the device `selected` is read there."""
        c = self.num_classes
        if self.device is not None:
            from ._lib import lib, check
            from .ops import ptr, stream_ptr
            args = (ptr(filtered), ptr(selected), ptr(self._start), self.K) + tuple(filtered.shape)
            if c:
                check(lib.aide_label_bank_update_classes(*args, ptr(self._palette), c, ptr(plane), stream_ptr()),
                      'label_bank_update_classes')
            else:
                check(lib.aide_label_bank_update(*args, LIVER, ptr(plane), stream_ptr()), 'label_bank_update')
            return
        lut = (np.arange(256) * LIVER).astype(np.uint8)
        if c:
            lut[:] = self.palette[0]
            lut[:c] = self.palette
        for k in np.flatnonzero(selected):
            a, b = self.slice_start[k], self.slice_start[k + 1]
            plane[a:b] = lut[filtered[a:b]]

    def refresh(self, net1, net2, inputs, epoch, warmup_epoch, batch_size=16, views=None):
        """inputs = (inphase[, outphase]), each [S_total,3,H,W]: both networks (eval mode) predict every slice, then
        `refresh_from_labels`.  `predict_labels` is `label_map`, the arg-max over however many channels the network has
        (2 .. 8), so a C-class network already yields the class maps the num_classes=C bank expects.  views: the test-time
        augmentation of `predict_labels` for each network (None: the single forward)."""
        return self.refresh_from_labels(predict_labels(net1, *inputs, batch_size=batch_size, views=views),
                                        predict_labels(net2, *inputs, batch_size=batch_size, views=views), epoch, warmup_epoch)

    def case_dice(self):
        """float32 [2,K] on the host -- traincasedices1 / traincasedices2 of the last refresh (:488-489): ONE device-to-host copy.
        The epoch's numbers are then `d[n].sum() / float(K)` on the host as :495-496."""
        return self._dice.cpu() if self.device is not None else torch.from_numpy(self._dice.copy())

    def class_dice(self):
        """float32 [2,K,C] on the host -- the per-class Dice of the last refresh, background included (NaN where a class is
        in neither the prediction nor the pseudo-label): ONE device-to-host copy.  Needs num_classes."""
        if self.num_classes is None:
            raise RuntimeError('PseudoLabelBank.class_dice: the bank was made without num_classes')
        return self._class_dice.cpu() if self.device is not None else torch.from_numpy(self._class_dice.copy())

    def modify_list(self, net):
        """the cases of the reference's 'Mask [...] modify for netN' line (:552, :575): the first int(0.25 * K) cases in
        ascending Dice, labelled ones included (they are listed but not rewritten).  Copies the ranks to the host."""
        rank = self.rank[net - 1]
        rank = rank.cpu().numpy() if self.device is not None else rank
        order = np.argsort(rank, kind='stable')[:self.n_select]
        return [self.case_ids[int(k)] for k in order]

    # ---- next epoch ----
    def targets(self, slice_idx, net, index=False, ignore_index=255):
        """one-hot int64 [N,P,H,W] over the palette of network `net`'s (1 or 2) pseudo-labels for the slices `slice_idx`:
        the loader's mask1 / mask2 (dataset.py:95-105), so `targets(...)[:, 1]` is the step's target.
        index=True: int64 [N,H,W] class indices instead, the target form the fused multi-class losses take directly (8 bytes
        per pixel, not 8 * P): the position of every byte in the palette, `ignore_index` for a byte outside it, and a plane of
        `ignore_index` for a slice index outside the bank.  Needs 2 .. 8 distinct palette bytes."""
        if net not in (1, 2):
            raise ValueError('net must be 1 or 2')
        plane = self.bank[net - 1]
        if index and not (2 <= len(self.palette) <= 8 and len(set(self.palette)) == len(self.palette)):
            raise ValueError('PseudoLabelBank.targets(index=True): 2 .. 8 distinct palette bytes, got %r' % (self.palette,))
        if self.device is None:
            idx = np.asarray(slice_idx, np.int64).reshape(-1)
            if index:
                tbl = np.full(256, int(ignore_index), np.int64)
                tbl[list(self.palette)] = np.arange(len(self.palette))
                ok = (idx >= 0) & (idx < plane.shape[0])
                out = tbl[plane[np.where(ok, idx, 0)]] if plane.shape[0] else np.empty((len(idx),) + plane.shape[1:], np.int64)
                out[~ok] = int(ignore_index)
                return torch.from_numpy(out)
            sl = plane[idx]
            return torch.from_numpy(np.stack([(sl == p) for p in self.palette], axis=1).astype(np.int64))
        from ._lib import lib, check
        from .ops import ptr, stream_ptr
        idx = torch.as_tensor(slice_idx, dtype=torch.int64).reshape(-1)
        if not idx.is_cuda:
            idx = idx.pin_memory().to(self.device, non_blocking=True)
        _, h, w = plane.shape
        if index:
            out = torch.empty(idx.numel(), h, w, device=self.device, dtype=torch.int64)
            check(lib.aide_label_bank_targets_index(ptr(plane), *plane.shape, ptr(idx), idx.numel(), ptr(self._palette),
                                                    len(self.palette), int(ignore_index), ptr(out), stream_ptr()),
                  'label_bank_targets_index')
            return out
        out = torch.empty(idx.numel(), len(self.palette), h, w, device=self.device, dtype=torch.int64)
        check(lib.aide_label_bank_targets(ptr(plane), *plane.shape, ptr(idx), idx.numel(), ptr(self._palette),
                                          len(self.palette), ptr(out), stream_ptr()), 'label_bank_targets')
        return out

    # ---- interchange ----
    def export_png(self, root, names):
        """Writes the files the reference would have written so far: `<root>/<case id>/<names[s]>_net{1,2}.png` (mode L) for
        every slice s of every case that was rewritten for that network (:544-551).  Host side, through PIL.  -> the paths."""
        from PIL import Image
        if len(names) != self.slice_start[-1]:
            raise RuntimeError('export_png: %d names for %d slices' % (len(names), self.slice_start[-1]))
        bank = self.bank.cpu().numpy() if self.device is not None else self.bank
        mod = self.modified.cpu().numpy() if self.device is not None else self.modified
        written = []
        for n in (0, 1):
            for k in np.flatnonzero(mod[n]):
                folder = os.path.join(root, str(self.case_ids[k]))
                os.makedirs(folder, exist_ok=True)
                for s in range(self.slice_start[k], self.slice_start[k + 1]):
                    path = os.path.join(folder, '%s_net%d.png' % (names[s], n + 1))
                    Image.fromarray(bank[n, s], 'L').save(path)
                    written.append(path)
        return written


# scoring targets of the two networks: (network 1, network 2), each 'original' or the index of a bank plane.
#   breast: sample[2] = the original mask, sample[3] = network 1's pseudo-label (trainbreast_dataset3_proposed_272cases25labeled.py:380-381)
#   kidney: sample[4] = network 2's, sample[3] = network 1's (trainkidney_proposed_mask1.py:380-381)
IMAGE_FORMS = {
    'breast': dict(score=('original', 0), scale=255, gated=False, skip_labelled=True),
    'kidney': dict(score=(1, 0), scale=1, gated=True, skip_labelled=False),
}


class ImageLabelBank(object):
    """The per-IMAGE label self-correction of the kidney and breast scripts (trainkidney_proposed_mask{1,2,3}.py:373-434,
    trainbreast_dataset3_proposed_272cases25labeled.py:373-438).

    original_masks_u8: [K,H,W] uint8, the original mask of every training image; both pseudo-label planes start as copies
    of it (the loaders fall back to it while no `_net1` / `_net2` file exists).  labelled: indices of the images whose
    labels are never rewritten (breast: `maskname not in labeled_cases`, :411; the kidney scripts have no such exception
    and ignore it).  A HIP tensor (or device=...) keeps the bank on the device; numpy / CPU input keeps a numpy bank.

    The rule, for network n, image k, p = argmax(softmax(logits)) in {0, 1}, t = the scoring target:
      sums     sum p*t, sum p, sum t: exact integers
      dice     0.0 if sum p + sum t == 0 (Dice2d never gives NaN), else float32(float64(2 sum p*t) / float64(sum p + sum t))
      target   breast: network 1 against the ORIGINAL mask, network 2 against NETWORK 1's plane, t = byte > 0;
               kidney: network 1 against NETWORK 2's plane, network 2 against NETWORK 1's, t = (byte > 0) & gate[k], where
               gate[k] says that the original mask of image k is not constant: the kidney ToTensor multiplies every mask by
               len(np.unique(original mask)) - 1 (datasetkidney_proposed/transform.py:96-104), so an image with a constant
               original mask has all-zero targets whatever its pseudo-label planes hold
      order    all four score vectors are taken BEFORE either network's planes are rewritten (network 2 reads network 1's)
      ranking  ascending dice, equal values by the lower image index.  This is this project's rule: the reference's
               `Tensor.sort()` is not stable.  Ties at 0.0 are COMMON here (every empty prediction against an empty
               target scores 0.0), so which of them fall inside the worst n_select is decided by this rule, not by the reference
      select   n_select = int(update_percent * K), the float product truncated as Python does
      write    written[k] = rank[k] < n_select and sum p[k] > 0 (:418 `if save_data.sum() > 0`) [and not labelled[k]: breast]
               while `refresh_gate(epoch, warmup_epoch)` is open: plane_n[k] = p * scale (255: breast PNGs, 1: kidney volumes)

    The reference evaluates `train_dataset.__getitem__`, i.e. under the random training transform, and writes the labels in
    that frame; in which frame `inputs` and the planes are is the caller's business."""

    def __init__(self, original_masks_u8, labelled=None, form='breast', update_percent=0.25, device=None, image_ids=None):
        if form not in IMAGE_FORMS:
            raise ValueError("ImageLabelBank: form must be 'breast' or 'kidney'")
        self.form = form
        self._f = IMAGE_FORMS[form]
        m = original_masks_u8
        on_dev = isinstance(m, torch.Tensor) and m.is_cuda
        if device is None and on_dev:
            device = m.device
        self.device = torch.device(device) if device is not None else None
        if self.device is not None and self.device.type != 'cuda':
            self.device = None
        if m.dtype not in (torch.uint8, np.uint8) or len(m.shape) != 3:
            raise RuntimeError('ImageLabelBank: [K,H,W] uint8 masks expected')
        self.K, self.H, self.W = (int(v) for v in m.shape)
        if self.K > (1 << 20):
            raise RuntimeError('ImageLabelBank: %d images, at most 2^20' % self.K)
        self.update_percent = float(update_percent)
        self.n_select = int(self.update_percent * self.K)        # :403 / :406
        if self.n_select < 0:
            raise ValueError('ImageLabelBank: update_percent must not be negative')
        lab = np.zeros(self.K, np.uint8)
        if self._f['skip_labelled']:
            for k in (labelled if labelled is not None else ()):
                lab[int(k)] = 1
        self.labelled_host = lab
        self.image_ids = list(image_ids) if image_ids is not None else None
        if self.image_ids is not None and len(self.image_ids) != self.K:
            raise RuntimeError('ImageLabelBank: %d image ids for %d images' % (len(self.image_ids), self.K))
        host = np.ascontiguousarray(m.cpu().numpy() if isinstance(m, torch.Tensor) else m)
        flat = host.reshape(self.K, -1)
        # computed once, from the ORIGINAL masks: len(np.unique(mask)) - 1 of the thresholded (0 / 255) mask is 1 or 0
        gate = ((flat > 0).any(1) & (flat == 0).any(1)).astype(np.uint8) if flat.shape[1] else np.zeros(self.K, np.uint8)
        self.gate_host = gate if self._f['gated'] else None
        if self.device is not None:
            dev = self.device
            self.original = torch.as_tensor(m).to(dev).contiguous()
            self.bank = torch.stack([self.original, self.original]).contiguous()
            self._labelled = torch.from_numpy(lab).to(dev) if self._f['skip_labelled'] else None
            self._gate = torch.from_numpy(gate).to(dev) if self._f['gated'] else None
            self._pred = torch.zeros(2, self.K, self.H, self.W, device=dev, dtype=torch.uint8)
            self._sums = torch.zeros(2, self.K, 4, device=dev, dtype=torch.int64)
            self._dice = torch.zeros(2, self.K, device=dev, dtype=torch.float32)
            self.rank = torch.zeros(2, self.K, device=dev, dtype=torch.int32)
            self.written = torch.zeros(2, self.K, device=dev, dtype=torch.uint8)
            self.modified = torch.zeros(2, self.K, device=dev, dtype=torch.uint8)
        else:
            self.original = host.copy()
            self.bank = np.stack([host, host])
            self._pred = np.zeros((2, self.K, self.H, self.W), np.uint8)
            self._sums = np.zeros((2, self.K, 4), np.int64)
            self._dice = np.zeros((2, self.K), np.float32)
            self.rank = np.zeros((2, self.K), np.int32)
            self.written = np.zeros((2, self.K), np.uint8)
            self.modified = np.zeros((2, self.K), np.uint8)

    def _score_plane(self, n):
        s = self._f['score'][n]
        return self.original if s == 'original' else self.bank[s]

    # ---- epoch end ----
    def _finish(self, epoch, warmup_epoch):
        """Dice, ranking and write flags of both networks from the sums, THEN (gate open) the rewrite of both planes"""
        write = refresh_gate(epoch, warmup_epoch)
        if self.device is not None:
            from .inference import image_refresh_select, image_bank_update
            for n in (0, 1):
                image_refresh_select(self._sums[n], self._labelled, self.n_select, out=(self._dice[n], self.rank[n], self.written[n]))
            if write:
                for n in (0, 1):
                    image_bank_update(self._pred[n], self.written[n], self._f['scale'], self.bank[n])
                self.modified.bitwise_or_(self.written)
        else:
            from .inference import image_dice_rule
            for n in (0, 1):
                self._dice[n], self.rank[n], self.written[n] = image_dice_rule(self._sums[n], self.labelled_host, self.n_select)
            if write:
                for n in (0, 1):
                    w = self.written[n].astype(bool)
                    self.bank[n][w] = self._pred[n][w] * np.uint8(self._f['scale'])       # :417-420 / :416-419
                self.modified |= self.written
        return write

    def _host_sums(self, n, labels):
        p = (np.asarray(labels) != 0).reshape(self.K, -1)
        t = (self._score_plane(n) > 0).reshape(self.K, -1)
        if self.gate_host is not None:
            t = t & self.gate_host.astype(bool)[:, None]
        self._pred[n] = p.reshape(self.K, self.H, self.W).astype(np.uint8)
        self._sums[n, :, 0] = self.H * self.W
        self._sums[n, :, 1] = (p & t).sum(1, dtype=np.int64)
        self._sums[n, :, 2] = p.sum(1, dtype=np.int64)
        self._sums[n, :, 3] = t.sum(1, dtype=np.int64)

    def refresh_from_labels(self, labels1, labels2, epoch, warmup_epoch, batch_size=4096):
        """labels1 / labels2: the two networks' label maps [K,H,W] (uint8 or int64, values 0 / 1) of all images.  Dice and
        ranking are taken every epoch, from planes as they were BEFORE this call; the planes are rewritten only while the
        gate is open.  -> whether it was.  On the device: no host synchronisation (`written` never leaves it)."""
        if self.device is None:
            for n, labels in enumerate((labels1, labels2)):
                labels = labels.numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
                if tuple(labels.shape) != (self.K, self.H, self.W):
                    raise RuntimeError('ImageLabelBank: label maps [%d,%d,%d] expected' % (self.K, self.H, self.W))
                self._host_sums(n, labels)
            return self._finish(epoch, warmup_epoch)
        from .inference import image_eval_labels
        for n, labels in enumerate((labels1, labels2)):
            if not (isinstance(labels, torch.Tensor) and labels.is_cuda and tuple(labels.shape) == (self.K, self.H, self.W)):
                raise RuntimeError('ImageLabelBank: the bank is on %s, the label maps [K,H,W] must be too' % self.device)
            if labels.dtype not in (torch.uint8, torch.int64):
                labels = labels.to(torch.int64)
            plane = self._score_plane(n)
            for i in range(0, self.K, batch_size):
                image_eval_labels(labels[i:i + batch_size], plane[i:i + batch_size], self._gate, i, self._pred[n], self._sums[n])
        return self._finish(epoch, warmup_epoch)

    def refresh(self, net1, net2, inputs, epoch, warmup_epoch, batch_size=16):
        """inputs: [K,3,H,W] (or a 1-tuple of it): both networks (eval mode) predict every image in batches; the logits of a
        batch go straight through the fused epilogue (labels as uint8 + exact sums: no int64 label tensor of [K,H,W] exists),
        then the rule.  Nothing synchronises with the host between prediction and update."""
        if self.device is None:
            raise RuntimeError('ImageLabelBank.refresh predicts on the device; a numpy bank takes refresh_from_labels')
        from .inference import image_eval_logits
        x = inputs[0] if isinstance(inputs, (tuple, list)) else inputs
        if x.shape[0] != self.K or tuple(x.shape[-2:]) != (self.H, self.W):
            raise RuntimeError('ImageLabelBank.refresh: inputs [%d,3,%d,%d] expected' % (self.K, self.H, self.W))
        for n, net in enumerate((net1, net2)):
            if net.training:
                raise RuntimeError('ImageLabelBank.refresh needs net.eval(), as predict_labels does (:345-346)')
            plane = self._score_plane(n)
            with torch.no_grad():
                for i in range(0, self.K, batch_size):
                    logits = net(x[i:i + batch_size].to(self.device, non_blocking=True))
                    image_eval_logits(logits, plane[i:i + batch_size], self._gate, i, self._pred[n], self._sums[n])
        return self._finish(epoch, warmup_epoch)

    def image_dice(self):
        """float32 [2,K] on the host -- traindices1 / traindices2 of the last refresh (:392-393): ONE device-to-host copy.  The
        epoch's numbers are then `d[n].sum() / float(K)` on the host (evaltrainavgdice1 / 2, :396-397)."""
        return self._dice.cpu() if self.device is not None else torch.from_numpy(self._dice.copy())

    def modify_count(self, net):
        """the number of the reference's '{} masks modified for netN' line (:421, :438): len(sortidx[:n_select]), images that
        were skipped (labelled, empty prediction) included.  No device read."""
        if net not in (1, 2):
            raise ValueError('net must be 1 or 2')
        return min(self.n_select, self.K)

    def written_images(self, net):
        """indices of the images whose plane the last refresh rewrote (or would have, gate closed).  Copies K bytes."""
        w = self.written[net - 1]
        return np.flatnonzero(w.cpu().numpy() if self.device is not None else w).tolist()

    # ---- next epoch ----
    def targets(self, idx, net):
        """int64 [N,H,W] targets of network `net`'s (1 or 2) pseudo-labels for the images `idx`: the loaders' mask1 / mask2
        after ToTensor -- breast `byte > 0`, kidney `(byte > 0) & gate`.  An index outside [0, K) gives zeros."""
        if net not in (1, 2):
            raise ValueError('net must be 1 or 2')
        plane = self.bank[net - 1]
        if self.device is None:
            idx = np.asarray(idx, np.int64).reshape(-1)
            ok = (idx >= 0) & (idx < self.K)
            t = plane[np.where(ok, idx, 0)] > 0
            t &= ok[:, None, None]
            if self.gate_host is not None:
                t &= self.gate_host.astype(bool)[np.where(ok, idx, 0)][:, None, None]
            return torch.from_numpy(t.astype(np.int64))
        from ._lib import lib, check
        from .ops import ptr, stream_ptr
        idx = torch.as_tensor(idx, dtype=torch.int64).reshape(-1)
        if not idx.is_cuda:
            idx = idx.pin_memory().to(self.device, non_blocking=True)
        out = torch.empty(idx.numel(), self.H, self.W, device=self.device, dtype=torch.int64)
        check(lib.aide_image_bank_targets(ptr(plane), self.K, self.H, self.W, ptr(idx), idx.numel(),
                                          ptr(self._gate) if self._gate is not None else None, ptr(out), stream_ptr()),
              'image_bank_targets')
        return out

    # ---- interchange ----
    def export(self, root, writer=None):
        """Writes the files the reference would have written so far, for every image that was rewritten for a network.
        breast: `<root>/<caseid>/<caseid>_depth<d>_net{1,2}.png` through PIL (:412-420), image_ids[k] = (caseid, depth).
        kidney: `writer(path, array)` with path `<root>/<folder>/<stem>_net{1,2}.nii.gz` and the int64 [1,H,W] array the
        reference hands to SimpleITK (:412-419), image_ids[k] = (folder, stem); the caller supplies the writer.  -> the paths."""
        ids = self.image_ids
        if ids is None:
            ids = [(str(k), 0) for k in range(self.K)] if self.form == 'breast' else [('0', str(k)) for k in range(self.K)]
        if self.form == 'kidney' and writer is None:
            raise RuntimeError('ImageLabelBank.export: the kidney form needs a writer(path, array)')
        bank = self.bank.cpu().numpy() if self.device is not None else self.bank
        mod = self.modified.cpu().numpy() if self.device is not None else self.modified
        paths = []
        for n in (0, 1):
            for k in np.flatnonzero(mod[n]):
                a, b = ids[k]
                folder = os.path.join(root, str(a))
                os.makedirs(folder, exist_ok=True)
                if self.form == 'breast':
                    from PIL import Image
                    path = os.path.join(folder, '%s_depth%s_net%d.png' % (a, b, n + 1))
                    Image.fromarray(bank[n, k]).save(path)
                else:
                    path = os.path.join(folder, '%s_net%d.nii.gz' % (b, n + 1))
                    writer(path, bank[n, k][None].astype(np.int64))
                paths.append(path)
        return paths
