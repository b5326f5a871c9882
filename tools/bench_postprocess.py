"""Case post-processing on the device: the k largest blobs per class and hole filling vs the existing filters and vs the host.
usage (GPU box): python tools/bench_postprocess.py [--out profiles/r16_postprocess.txt]

A synthetic five-class volume (background + four organs, several blobs per class, a few hundred speckles; every large organ
has cavities: a few ellipsoidal ones and some hundred single voxels) at 256^2 x 33 and at 512^2 x 100; timed in one process:
  top-2        aide_amd.inference.keep_components(volume, top_k=2, num_classes=5) on the HIP tensor (device events around the
               call: the memset, the three labelling kernels, two select passes, write)
  per class    keep_largest_per_class(volume, 5), the existing filter on the same volume (one select pass)
  fill         fill_holes(volume, 5) (3-D) and fill_holes(volume, 5, slice_axis=2): the memset, the labelling kernels on the
               background, flag, write
  complement   keep_largest_connected_components(volume == 0): the existing binary filter on the complement volume, which is
               the same labelling work over the same voxels
  host         the numpy paths of keep_components and fill_holes (scipy.ndimage.label; host clock)
Medians after warm-up; ratios = top-2 / per class and fill / complement.  Nothing here is a gate.  Under the table the launches
of one fill_holes call and of one complement call are timed one by one with the library's kernel timer (begin / end of every
dispatch), so that the file says which launch takes the time when fill takes more than twice the complement filter.  The
device results are compared with the host's before anything is timed."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aide_amd.inference import (keep_largest_connected_components as keep, keep_largest_per_class, keep_components,
                                fill_holes)

SHAPES = ((256, 256, 33), (512, 512, 100))
C = 5


def organs(h, w, s, rng):
    """[H,W,S] int64 labels 0 .. 4: per class one large ellipsoid, two smaller ones and 75 speckles of 1 - 4 voxels; then
    cavities: per class three ellipsoids of zeros inside the large one and single zero voxels at 0.5 % of the volume"""
    yy, xx, zz = np.meshgrid(np.arange(h), np.arange(w), np.arange(s), indexing='ij', sparse=True)
    v = np.zeros((h, w, s), np.int64)
    big = []
    for c in range(1, C):
        for scale in (0.16, 0.07, 0.05):
            cy, cx, cz = rng.uniform(0.15, 0.85) * h, rng.uniform(0.15, 0.85) * w, rng.uniform(0.2, 0.8) * s
            ry, rx, rz = scale * h * rng.uniform(0.7, 1.3), scale * w * rng.uniform(0.7, 1.3), 2.5 * scale * s
            v[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 + ((zz - cz) / rz) ** 2 <= 1.0] = c
            if scale == 0.16:
                big.append((cy, cx, cz, ry, rx, rz))
        for _ in range(75):
            y, x, z = rng.randint(0, h - 2), rng.randint(0, w - 2), rng.randint(0, s)
            v[y:y + 1 + rng.randint(2), x:x + 1 + rng.randint(2), z] = c
    for cy, cx, cz, ry, rx, rz in big:
        for _ in range(3):
            oy, ox, oz = (rng.uniform(-0.5, 0.5) * r for r in (ry, rx, rz))
            v[((yy - cy - oy) / (0.2 * ry)) ** 2 + ((xx - cx - ox) / (0.2 * rx)) ** 2 + ((zz - cz - oz) / (0.2 * rz)) ** 2 <= 1.0] = 0
    v[rng.rand(h, w, s) < 0.005] = 0
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


def launch_split(fn):
    """the durations in ms of the launches of one call, in launch order"""
    from aide_amd.profiling import DispatchTimer
    torch.cuda.synchronize()
    timer = DispatchTimer(32, families=[15])
    timer.start()
    try:
        fn()
    finally:
        timer.stop()
    return [row['t1'] - row['t0'] for row in timer.timeline()]


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

    rng = np.random.RandomState(12)
    splits = []
    out('# k largest blobs per class and hole filling (C = %d) vs the existing filters vs the host paths (%s)' % (
        C, torch.cuda.get_device_name(0)))
    out('%-12s %6s %-22s %9s %12s %7s | %-16s %8s %9s %13s %7s %9s | %9s %9s' % (
        'shape', 'bg %', 'holes filled 3-D / ax2', 'top-2 ms', 'per class ms', 'ratio', 'voxels filled', 'fill ms', 'fill2 ms',
        'complement ms', 'ratio', 'ratio ax2', 'host top2', 'host fill'))
    for shape in SHAPES:
        v = organs(*shape, rng)
        t = torch.from_numpy(v).to(dev)
        comp = (t == 0).to(torch.int64)
        t0 = time.perf_counter()
        ref_k, ref_ks = keep_components(v, 2, 1, C, stats=True)
        ref_f, ref_fs = fill_holes(v, C, stats=True)
        ref_f2, ref_fs2 = fill_holes(v, C, 2, stats=True)
        one = (time.perf_counter() - t0) / 3
        for got, want in ((keep_components(t, 2, 1, C, stats=True), (ref_k, ref_ks)), (fill_holes(t, C, stats=True), (ref_f, ref_fs)),
                          (fill_holes(t, C, 2, stats=True), (ref_f2, ref_fs2))):
            assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]), shape
        t_top = med_device(lambda: keep_components(t, 2, 1, C))
        t_cls = med_device(lambda: keep_largest_per_class(t, C))
        t_fill = med_device(lambda: fill_holes(t, C))
        t_fill2 = med_device(lambda: fill_holes(t, C, 2))
        t_comp = med_device(lambda: keep(comp))
        n_host = 10 if one < 1.0 else 3
        h_top = med_host(lambda: keep_components(v, 2, 1, C), n_host)
        h_fill = med_host(lambda: fill_holes(v, C), n_host)
        out('%-12s %6.1f %-22s %9.3f %12.3f %7.2f | %-16s %8.3f %9.3f %13.3f %7.2f %9.2f | %9.1f %9.1f' % (
            'x'.join(map(str, shape)), 100.0 * (v == 0).sum() / v.size, '%d / %d' % (ref_fs[:, 0].sum(), ref_fs2[:, 0].sum()),
            t_top, t_cls, t_top / t_cls, '%d / %d' % (ref_fs[:, 1].sum(), ref_fs2[:, 1].sum()), t_fill, t_fill2, t_comp,
            t_fill / t_comp, t_fill2 / t_comp, h_top, h_fill))
        splits.append((shape, launch_split(lambda: fill_holes(t, C)), launch_split(lambda: fill_holes(t, C, 2)),
                       launch_split(lambda: keep(comp)), t_fill / t_comp))
        del t, comp
    out()
    out('# one call, launch by launch, ms (fill: local, border, count, flag, write; complement: local, border, count, select, write)')
    for shape, f3, f2, cp, ratio in splits:
        tag = 'x'.join(map(str, shape))
        out('%-12s fill        %s' % (tag, ' '.join('%7.3f' % x for x in f3)))
        out('%-12s fill ax2    %s' % (tag, ' '.join('%7.3f' % x for x in f2)))
        out('%-12s complement  %s' % (tag, ' '.join('%7.3f' % x for x in cp)))
        if ratio > 2.0 and len(f3) == 5:
            names = ('local', 'border', 'count', 'flag', 'write')
            out('%-12s fill takes %.2f times the complement filter: the %s launch takes the most time' % (
                tag, ratio, names[int(np.argmax(f3))]))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
