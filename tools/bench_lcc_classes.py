"""Per-class largest-component filter on the device vs the binary filter and vs the host definition.
usage (GPU box): python tools/bench_lcc_classes.py [--out profiles/r12_lcc_classes.txt]

A synthetic five-class volume (background + four organs, several blobs per class, a few hundred speckles) at 256^2 x 33 and
at 512^2 x 100; timed in one process:
  classes      aide_amd.inference.keep_largest_per_class(volume, 5) on the HIP tensor (device events around the call: one
               memset + the five kernels of aide_keep_largest_cc3d_classes), without and with stats
  binary       keep_largest_connected_components(volume != 0) on the HIP tensor: the existing one-blob filter on the same
               foreground, whose first three kernels are the ones the per-class form launches too
  host         keep_largest_per_class on the numpy array (scipy.ndimage.label once per class; host clock)
Medians after warm-up; ratio = classes / binary.  The device result is compared with the host's before anything is timed."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aide_amd.inference import keep_largest_connected_components as keep, keep_largest_per_class

SHAPES = ((256, 256, 33), (512, 512, 100))
C = 5


def organs(h, w, s, rng):
    """[H,W,S] int64 labels 0 .. 4: per class one large ellipsoid, two smaller ones, and 75 speckles of 1 - 4 voxels"""
    yy, xx, zz = np.meshgrid(np.arange(h), np.arange(w), np.arange(s), indexing='ij', sparse=True)
    v = np.zeros((h, w, s), np.int64)
    for c in range(1, C):
        for scale in (0.16, 0.07, 0.05):
            cy, cx, cz = rng.uniform(0.15, 0.85) * h, rng.uniform(0.15, 0.85) * w, rng.uniform(0.2, 0.8) * s
            ry, rx, rz = scale * h * rng.uniform(0.7, 1.3), scale * w * rng.uniform(0.7, 1.3), 2.5 * scale * s
            v[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 + ((zz - cz) / rz) ** 2 <= 1.0] = c
        for _ in range(75):
            y, x, z = rng.randint(0, h - 2), rng.randint(0, w - 2), rng.randint(0, s)
            v[y:y + 1 + rng.randint(2), x:x + 1 + rng.randint(2), z] = c
    return v


def med_device(fn, reps=25, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def med_host(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = []

    def out(s=''):
        print(s, flush=True)
        lines.append(s)

    out('# largest component per class (C = %d) vs the binary filter vs the host definition (%s)' % (
        C, torch.cuda.get_device_name(0)))
    out('%-12s %6s %-24s %11s %11s %10s %8s %10s %6s %9s' % ('shape', 'fg %', 'blobs per class 1..4', 'classes ms', '+stats ms',
                                                           'binary ms', 'ratio', 'host ms', 'host n', 'speed-up'))
    rng = np.random.RandomState(12)
    for shape in SHAPES:
        v = organs(*shape, rng)
        t = torch.from_numpy(v).to(dev)
        fg = (t != 0).to(torch.int64)
        t0 = time.perf_counter()
        ref, ref_stats = keep_largest_per_class(v, C, stats=True)
        one = time.perf_counter() - t0
        got, stats = keep_largest_per_class(t, C, stats=True)
        assert np.array_equal(got.cpu().numpy(), ref) and np.array_equal(stats.cpu().numpy(), ref_stats), shape
        assert np.array_equal(keep(fg).cpu().numpy(), keep(v != 0)), shape
        t_cls = med_device(lambda: keep_largest_per_class(t, C))
        t_st = med_device(lambda: keep_largest_per_class(t, C, stats=True))
        t_bin = med_device(lambda: keep(fg))
        n_host = 10 if one < 1.0 else 3
        t_host = med_host(lambda: keep_largest_per_class(v, C), n_host)
        out('%-12s %6.1f %-24s %11.3f %11.3f %10.3f %8.2f %10.1f %6d %8.0fx' % (
            'x'.join(map(str, shape)), 100.0 * np.count_nonzero(v) / v.size, ' '.join(str(int(x)) for x in ref_stats[1:, 0]),
            t_cls, t_st, t_bin, t_cls / t_bin, t_host, n_host, t_host / t_cls))
        del t, fg
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
