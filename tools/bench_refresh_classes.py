"""Multi-organ pseudo-label refresh (C = 5) on the device vs the binary refresh and vs the numpy bank.
usage (GPU box): python tools/bench_refresh_classes.py [--out profiles/r14_refresh_classes.txt]

Label maps of `chaos_cases_multiorgan` at 256^2 x 33 x 30 cases (six drawn cases, shifted copies up to thirty: the drawing is
host time), two networks' maps = the truth's class indices shifted by a few pixels with 1 % speckle.  Timed in one process,
the forms alternating inside every repetition, the bank restored before each timed call:
  classes      PseudoLabelBank(num_classes=5).refresh_from_labels, gate open, both networks (per network: the per-class
               filter, aide_case_class_counts_batched, aide_label_refresh_select_classes, aide_label_bank_update_classes)
  binary       PseudoLabelBank().refresh_from_labels on `map != 0` against `initial != 0` of the same cases (the one-blob
               filter, aide_case_confusion_batched, aide_label_refresh_select, aide_label_bank_update)
  no filter    both again with keep_largest=False on uint8 maps (no cast): counts / sums, rule and update alone, the part
               that reads the label and the bank bytes about once in either form
  host         the numpy bank (scipy filter per case and class), host clock
Device events around each call, medians after warm-up; ratio = classes / binary.  The device bank is compared with the numpy
bank byte for byte, and the scores bit for bit, before anything is timed."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aide_amd.labelbank import PseudoLabelBank, CHAOS_PALETTE
from aide_amd.synthetic import chaos_cases_multiorgan

C = 5


def case_set(size, slices, cases, drawn=6):
    """-> (initial bank bytes u8 [S,H,W], two label maps int64 [S,H,W], slice_start)"""
    cs = chaos_cases_multiorgan(min(drawn, cases), C, size, seed=14, slices=(slices, slices), labelled=(0,))
    truth, init = cs['truth'].numpy(), cs['initial'].numpy()
    reps = -(-cases * slices // truth.shape[0])
    truth = np.concatenate([np.roll(truth, 3 * r, 2) for r in range(reps)])[:cases * slices]
    init = np.concatenate([np.roll(init, 3 * r, 2) for r in range(reps)])[:cases * slices]
    idx = np.zeros(truth.shape, np.uint8)
    for c in range(C):
        idx[truth == CHAOS_PALETTE[c]] = c
    rng = np.random.RandomState(3)
    maps = []
    for n in range(2):
        m = np.roll(idx, (2 + n, -3), (1, 2))
        noise = rng.rand(*m.shape) < 0.01
        maps.append(np.where(noise, rng.randint(0, C, m.shape), m).astype(np.int64))
    return init, maps, [k * slices for k in range(cases + 1)]


def med_device(fns, restore, reps, warm=2):
    """median device milliseconds of each fn, alternating; restore() runs before every timed call, outside the events"""
    ts = [[] for _ in fns]
    for r in range(warm + reps):
        for i, fn in enumerate(fns):
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warm:
                ts[i].append(e0.elapsed_time(e1))
    return [(float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--slices', type=int, default=33)
    ap.add_argument('--cases', type=int, default=30)
    ap.add_argument('--reps', type=int, default=15)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = []

    def out(s=''):
        print(s, flush=True)
        lines.append(s)

    init, maps, st = case_set(a.size, a.slices, a.cases)
    print('cases drawn', flush=True)
    init_d = torch.from_numpy(init).to(dev)
    maps_d = [torch.from_numpy(m).to(dev) for m in maps]
    bin_init_d = (init_d != 0).to(torch.uint8) * 63
    bin_maps_d = [(m != 0).to(torch.int64) for m in maps_d]
    cls = PseudoLabelBank(init_d, st, [0], num_classes=C)
    bnr = PseudoLabelBank(bin_init_d, st, [0])
    host = PseudoLabelBank(init, st, [0], num_classes=C)

    t0 = time.perf_counter()
    host.refresh_from_labels(maps[0], maps[1], 0, 1)
    t_host = (time.perf_counter() - t0) * 1e3
    print('numpy bank refreshed in %.0f ms' % t_host, flush=True)
    cls.refresh_from_labels(maps_d[0], maps_d[1], 0, 1)
    same = (np.array_equal(cls.bank.cpu().numpy(), host.bank)
            and np.array_equal(cls.case_dice().numpy().view(np.uint32), host.case_dice().numpy().view(np.uint32))
            and np.array_equal(cls.class_dice().numpy().view(np.uint32), host.class_dice().numpy().view(np.uint32))
            and np.array_equal(cls.rank.cpu().numpy(), host.rank))
    assert same, 'the device bank and the numpy bank differ'
    rewritten = int(cls.selected.sum().item())

    maps_u8, bin_u8 = [m.to(torch.uint8) for m in maps_d], [m.to(torch.uint8) for m in bin_maps_d]
    cls_init, bnr_init = torch.stack([init_d, init_d]), torch.stack([bin_init_d, bin_init_d])

    def restore():
        cls.bank.copy_(cls_init)
        bnr.bank.copy_(bnr_init)

    fns = [lambda: cls.refresh_from_labels(maps_d[0], maps_d[1], 0, 1),
           lambda: bnr.refresh_from_labels(bin_maps_d[0], bin_maps_d[1], 0, 1),
           lambda: cls.refresh_from_labels(maps_u8[0], maps_u8[1], 0, 1, keep_largest=False),
           lambda: bnr.refresh_from_labels(bin_u8[0], bin_u8[1], 0, 1, keep_largest=False)]
    r = med_device(fns, restore, a.reps)
    nbytes = 2 * 2 * init.size                              # both networks, label byte + bank byte per voxel
    out('# multi-organ refresh (C = %d) vs the binary refresh vs the numpy bank (%s)' % (C, torch.cuda.get_device_name(0)))
    out('# %d cases of %dx%dx%d, both networks, %d cases rewritten; device bank == numpy bank: %s; %d alternating repetitions'
        % (a.cases, a.size, a.size, a.slices, rewritten, same, a.reps))
    out('%-34s %10s %10s %10s' % ('form', 'median ms', 'min', 'max'))
    names = ('classes: filter + refresh', 'binary:  filter + refresh', 'classes: no filter', 'binary:  no filter')
    for name, (m, lo, hi) in zip(names, r):
        out('%-34s %10.3f %10.3f %10.3f' % (name, m, lo, hi))
    out('ratio classes / binary, with filter  %.2f' % (r[0][0] / r[1][0]))
    out('ratio classes / binary, no filter    %.2f' % (r[2][0] / r[3][0]))
    out('# no filter: %.1f MB of label and bank bytes, each read once by the counts, = %.0f / %.0f GB/s over the whole call'
        % (nbytes / 1e6, nbytes / r[2][0] / 1e6, nbytes / r[3][0] / 1e6))
    out('#   (the call also holds the rule, the rewrite of the selected cases and the gaps between its launches)')
    out('numpy bank (scipy filter per case and class), one call, host clock: %.0f ms = %.0fx the device call'
        % (t_host, t_host / r[0][0]))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
