"""Ball morphology and the distance transform on the device vs fill_holes on the same volume and vs scipy on the host.
usage (GPU box): python tools/bench_morphology.py [--out profiles/r19_morphology.txt]

The synthetic five-class cavity volume of tools/bench_postprocess.py at 256^2 x 33 and at 512^2 x 100, spacing 1.37 x 1.37 x 7.7 mm
(windows 2, 2, 0 at r = 3 mm and 7, 7, 1 at r = 10 mm).  Variants, timed in one process with device events around the public call
(workspace allocation included), ALTERNATING: every round times each variant once, medians over the rounds after warm-up:
  open / close at r = 3 and r = 10, binary and C = 5     aide_amd.morphology.open_ / close
  edt                                                    distance_transform of the same volume (binary foreground)
  fill                                                   aide_amd.inference.fill_holes(volume, 5)
  host                                                   the numpy path (scipy.ndimage, host clock, one run; C = 5 and r = 10 only
                                                         where it ends in reasonable time)
Effective TB/s = compulsory bytes / time, with the bytes per voxel stated next to it: a primitive (scan, mid, last) reads 1 and
writes 4, reads 4 and writes 8, reads 8 and writes 1 = 26 B; an opening or closing is two primitives per class plus the class map
(8 + 1 B for int64 labels, 1 more for the copy or memset of out): 62 B binary, 218 B for C = 5; the distance transform reads 8,
writes 1, reads 1 and writes 4, reads 4 and writes 8, reads 8 and writes 8 = 42 B.  Window re-reads are expected to hit the caches
and are not counted.  Nothing here is a gate except the one expectation from operation counts: an opening at r = 3 mm must take
less time than the distance transform; the file says so either way.  The device results are compared with the host's before
anything is timed."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from scipy import ndimage                         # imported here: the first host figure is not to hold the import

from aide_amd.inference import fill_holes
from aide_amd.morphology import open_, close, distance_transform
from bench_postprocess import organs, launch_split

SHAPES = ((256, 256, 33), (512, 512, 100))
SPACING = (1.37, 1.37, 7.7)
C = 5
B_BINARY, B_CLASSES, B_EDT = 10 + 2 * 26, 10 + 8 * 26, 42


def alternate(variants, rounds=15, warm=2):
    """{name: fn} -> {name: median ms}; every round runs each variant once, in order"""
    ts = {name: [] for name in variants}
    for k in range(warm + rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= warm:
                ts[name].append(e0.elapsed_time(e1))
    return {name: float(np.median(v)) for name, v in ts.items()}


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = []

    def out(s=''):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.RandomState(12)
    out('# ball morphology (spacing %s mm) and the distance transform vs fill_holes vs scipy on the host (%s)' % (
        ' x '.join(map(str, SPACING)), torch.cuda.get_device_name(0)))
    out('# ms = median of 15 alternating rounds; TB/s = voxels * B / time with B = %d (binary), %d (C = %d), %d (edt) bytes per voxel'
        % (B_BINARY, B_CLASSES, C, B_EDT))
    splits = []
    for shape in SHAPES:
        v = organs(*shape, rng)
        t = torch.from_numpy(v).to(dev)
        small = v.size < 2 ** 22
        host = {}
        for r in (3.0, 10.0):                     # the host runs double as the check of the device results
            for c in (None, C):
                if c is not None and not small:
                    continue
                for name, fn in (('open', open_), ('close', close)):
                    if name == 'close' and not (small and r == 3.0):
                        continue
                    box = []
                    host[(name, r, c)] = host_ms(lambda: box.append(fn(v, r, SPACING, c)))
                    assert np.array_equal(fn(t, r, SPACING, c).cpu().numpy(), box[0]), (shape, name, r, c)
        box = []
        host['edt'] = host_ms(lambda: box.append(ndimage.distance_transform_edt(v != 0, sampling=SPACING)))
        got = distance_transform(t, SPACING).cpu().numpy()
        assert np.all(np.abs(got - box[0]) <= 2.0 ** -49 * box[0]), shape
        host['fill'] = host_ms(lambda: fill_holes(v, C))
        variants = {}
        for r in (3.0, 10.0):
            for c in (None, C):
                for name, fn in (('open', open_), ('close', close)):
                    variants['%s r=%g %s' % (name, r, 'C=%d' % c if c else 'binary')] = \
                        (lambda fn=fn, r=r, c=c: fn(t, r, SPACING, c))
        variants['edt'] = lambda: distance_transform(t, SPACING)
        variants['fill'] = lambda: fill_holes(t, C)
        ms = alternate(variants)
        tag = 'x'.join(map(str, shape))
        out()
        out('%-12s %-20s %9s %7s %6s %10s' % ('shape', 'variant', 'ms', 'B/vox', 'TB/s', 'host ms'))
        for name, val in ms.items():
            b = B_EDT if name == 'edt' else None if name == 'fill' else B_CLASSES if 'C=' in name else B_BINARY
            parts = name.split()
            key = name if len(parts) == 1 else (parts[0], float(parts[1][2:]), C if 'C=' in name else None)
            h = host.get(key)
            out('%-12s %-20s %9.3f %7s %6s %10s' % (tag, name, val, b if b else '-',
                                                   '%.2f' % (v.size * b / (val * 1e-3) / 1e12) if b else '-',
                                                   '%.1f' % h if h is not None else '-'))
        verdict = 'less' if ms['open r=3 binary'] < ms['edt'] else 'NOT less'
        out('%-12s open r=3 binary takes %s time than edt: %.3f ms vs %.3f ms (%d candidate evaluations per voxel vs %d)' % (
            tag, verdict, ms['open r=3 binary'], ms['edt'], 2 * (5 + 5 + 1), shape[0] + shape[1]))
        splits.append((tag, launch_split(lambda: open_(t, 3.0, SPACING)), launch_split(lambda: open_(t, 10.0, SPACING)),
                       launch_split(lambda: distance_transform(t, SPACING))))
        del t
    out()
    out('# one call, launch by launch, ms (open: classes, then scan, mid, last of the erosion and of the dilation; '
        'edt: background, scan, d1, d0)')
    for tag, o3, o10, e in splits:
        out('%-12s open r=3     %s' % (tag, ' '.join('%7.3f' % x for x in o3)))
        out('%-12s open r=10    %s' % (tag, ' '.join('%7.3f' % x for x in o10)))
        out('%-12s edt          %s' % (tag, ' '.join('%7.3f' % x for x in e)))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
