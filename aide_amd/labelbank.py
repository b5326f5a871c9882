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
there."""
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
    A HIP tensor (or device=...) keeps the bank on the device; numpy / CPU input keeps a numpy bank."""

    def __init__(self, initial_masks_u8, slice_start, labelled_cases, palette=CHAOS_PALETTE, device=None, case_ids=None):
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
            self.rank = torch.zeros(2, self.K, device=self.device, dtype=torch.int32)
            self.selected = torch.zeros(2, self.K, device=self.device, dtype=torch.uint8)
            self.modified = torch.zeros(2, self.K, device=self.device, dtype=torch.uint8)
        else:
            m = np.ascontiguousarray(m.numpy() if isinstance(m, torch.Tensor) else m)
            self.bank = np.stack([m, m])
            self._dice = np.zeros((2, self.K), np.float32)
            self.rank = np.zeros((2, self.K), np.int32)
            self.selected = np.zeros((2, self.K), np.uint8)
            self.modified = np.zeros((2, self.K), np.uint8)

    # ---- epoch end ----
    def refresh_from_labels(self, labels1, labels2, epoch, warmup_epoch, keep_largest=True):
        """labels1 / labels2: the two networks' label maps [S_total,H,W] of all cases.  Case Dice and ranking are taken every
        epoch; the selected cases' planes are rewritten only while the gate of :528 is open.  -> whether it was.  On the
        device: no host synchronisation (`selected` never leaves it)."""
        from ._lib import lib, check
        from .ops import ptr, stream_ptr
        write = refresh_gate(epoch, warmup_epoch)
        for n, labels in enumerate((labels1, labels2)):
            if self.device is not None:
                if not (isinstance(labels, torch.Tensor) and labels.is_cuda):
                    raise RuntimeError('PseudoLabelBank: the bank is on %s, the label maps must be too' % self.device)
                r = evaluate_label_maps(labels, self._start, self.bank[n], self.match, self._labelled, self.n_select, keep_largest)
                self._dice[n].copy_(r['dice'])
                self.rank[n].copy_(r['rank'])
                self.selected[n].copy_(r['selected'])
                if write:
                    f = r['filtered']
                    check(lib.aide_label_bank_update(ptr(f), ptr(r['selected']), ptr(self._start), self.K, *f.shape, LIVER,
                                                     ptr(self.bank[n]), stream_ptr()), 'label_bank_update')
                    self.modified[n].bitwise_or_(r['selected'])
            else:
                r = evaluate_label_maps(np.asarray(labels), self.slice_start, self.bank[n], self.match, self.labelled_host,
                                        self.n_select, keep_largest)
                self._dice[n], self.rank[n], self.selected[n] = r['dice'], r['rank'], r['selected']
                if write:
                    for k in np.flatnonzero(r['selected']):
                        a, b = self.slice_start[k], self.slice_start[k + 1]
                        self.bank[n][a:b] = (r['filtered'][a:b] * LIVER).astype(np.uint8)     # :549-550
                    self.modified[n] |= r['selected']
        return write

    def refresh(self, net1, net2, inputs, epoch, warmup_epoch, batch_size=16):
        """inputs = (inphase[, outphase]), each [S_total,3,H,W]: both networks (eval mode) predict every slice, then
        `refresh_from_labels`."""
        return self.refresh_from_labels(predict_labels(net1, *inputs, batch_size=batch_size),
                                        predict_labels(net2, *inputs, batch_size=batch_size), epoch, warmup_epoch)

    def case_dice(self):
        """float32 [2,K] on the host -- traincasedices1 / traincasedices2 of the last refresh (:488-489): ONE device-to-host copy.
        The epoch's numbers are then `d[n].sum() / float(K)` on the host as :495-496."""
        return self._dice.cpu() if self.device is not None else torch.from_numpy(self._dice.copy())

    def modify_list(self, net):
        """the cases of the reference's 'Mask [...] modify for netN' line (:552, :575): the first int(0.25 * K) cases in
        ascending Dice, labelled ones included (they are listed but not rewritten).  Copies the ranks to the host."""
        rank = self.rank[net - 1]
        rank = rank.cpu().numpy() if self.device is not None else rank
        order = np.argsort(rank, kind='stable')[:self.n_select]
        return [self.case_ids[int(k)] for k in order]

    # ---- next epoch ----
    def targets(self, slice_idx, net):
        """one-hot int64 [N,P,H,W] over the palette of network `net`'s (1 or 2) pseudo-labels for the slices `slice_idx`:
        the loader's mask1 / mask2 (dataset.py:95-105), so `targets(...)[:, 1]` is the step's target."""
        if net not in (1, 2):
            raise ValueError('net must be 1 or 2')
        plane = self.bank[net - 1]
        if self.device is None:
            idx = np.asarray(slice_idx, np.int64).reshape(-1)
            sl = plane[idx]
            return torch.from_numpy(np.stack([(sl == p) for p in self.palette], axis=1).astype(np.int64))
        from ._lib import lib, check
        from .ops import ptr, stream_ptr
        idx = torch.as_tensor(slice_idx, dtype=torch.int64).reshape(-1)
        if not idx.is_cuda:
            idx = idx.pin_memory().to(self.device, non_blocking=True)
        _, h, w = plane.shape
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
