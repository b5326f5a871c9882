"""Times the multi-class metrics at the CHAOS mask shape (C = 5, N = 4, 256 x 256) on an MI355X.

    python tools/bench_metrics.py [--out profiles/r10_metrics.txt] [--iters 200]

Reported, each as the median of `--repeats` windows of `--iters` calls after a warm-up:
  MulticlassDice_fn      one call on HIP logits, wall clock (the call ends in its one device -> host copy, so it is complete)
  MulticlassMeter.update one call: host time to enqueue its two launches, and device time per call from events around a window
  host path              the same numbers from a CPU copy of the logits (`.cpu()` + arg-max + numpy counts), the shape of the
                         reference's own functions (utils/metrics2d.py:111-138), wall clock
  counts kernel          device time per call from events around a window of back-to-back launches, and the effective GB/s
                         against the bytes it must read (logits + targets; computed from the shapes here)
At this size the kernel moves ~16 MB; the last lines say whether the launch or the traffic bounds a call (the time the bytes
need at the HBM peak against the measured time per call) and repeat the kernel figure at N = 64, where the traffic dominates.
There is no CPU fall-back: without a HIP device the tool fails."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aide_amd.utils import MulticlassDice_fn, MulticlassMeter, multiclass_counts  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s (MI355X HBM3E peak)


def wall(fn, iters, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters)
    return statistics.median(out), min(out), max(out)


def device(fn, iters, repeats):
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3 / iters)
    return statistics.median(out), min(out), max(out)


def enqueue(fn, iters, repeats):
    """host time of the call alone: the queue is drained before and after the window, not inside it"""
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        out.append((time.perf_counter() - t0) / iters)
        torch.cuda.synchronize()
    return statistics.median(out), min(out), max(out)


def us(t):
    return '%9.2f us (min %.2f, max %.2f)' % (t[0] * 1e6, t[1] * 1e6, t[2] * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r10_metrics.txt'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--classes', type=int, default=5)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--size', type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_metrics: no HIP device; this tool measures on the GPU only')
    dev = torch.device('cuda:0')
    c, s = a.classes, a.size
    lines = ['multi-class metrics, C = %d, H x W = %d x %d, one-hot int64 targets (the loaders\' mask); %s'
             % (c, s, s, torch.cuda.get_device_name(0)),
             'median of %d windows of %d calls' % (a.repeats, a.iters)]

    def tensors(n):
        g = torch.Generator().manual_seed(7)
        x = torch.randn(n, c, s, s, generator=g)
        idx = torch.randint(0, c, (n, s, s), generator=g)
        onehot = torch.nn.functional.one_hot(idx, c).permute(0, 3, 1, 2).contiguous()
        return x, onehot

    x, onehot = tensors(a.batch)
    xd, td = x.to(dev), onehot.to(dev)
    assert np.array_equal(MulticlassDice_fn(xd, td), MulticlassDice_fn(x, onehot))
    meter = MulticlassMeter(c, dev)
    for _ in range(20):
        MulticlassDice_fn(xd, td)
        meter.update(xd, td)
    lines.append('N = %d' % a.batch)
    dice = wall(lambda: MulticlassDice_fn(xd, td), a.iters, a.repeats)
    lines.append('  MulticlassDice_fn (HIP logits, wall)          %s' % us(dice))
    lines.append('  MulticlassMeter.update, host enqueue          %s' % us(enqueue(lambda: meter.update(xd, td), a.iters, a.repeats)))
    lines.append('  MulticlassMeter.update, device per call       %s' % us(device(lambda: meter.update(xd, td), a.iters, a.repeats)))
    host = wall(lambda: MulticlassDice_fn(xd.cpu(), td.cpu()), max(a.iters // 20, 5), a.repeats)
    lines.append('  host path from a CPU copy of the logits       %s   (%.1f x MulticlassDice_fn on the device)'
                 % (us(host), host[0] / dice[0]))
    for n in (a.batch, 64):
        if n != a.batch:
            x, onehot = tensors(n)
            xd, td = x.to(dev), onehot.to(dev)
            for _ in range(20):
                multiclass_counts(xd, td)
        nbytes = n * s * s * c * (4 + 8)
        k = device(lambda: multiclass_counts(xd, td), a.iters, a.repeats)
        roof = nbytes / HBM_PEAK
        lines.append('  counts kernel N = %-3d %6.1f MB                %s   %.1f GB/s effective; the bytes need %.2f us at %.1f TB/s: '
                     '%s' % (n, nbytes / 1e6, us(k), nbytes / k[0] / 1e9, roof * 1e6, HBM_PEAK / 1e12,
                             'launch cost dominates' if k[0] > 2 * roof else 'traffic dominates'))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
