"""Surface distances (RAVD / ASSD / MSSD) on the device vs the host path.  usage (GPU box): python tools/bench_surface.py
[--out FILE]

Per shape, a filled ellipsoid against a shifted, dented copy (uint8 [H,W,S], spacing 1.37 x 1.37 x 7.7 mm):
  device  aide_amd.utils.metrics3d.surface_scores on HIP tensors -- (a) the five kernels of aide_surface3d_scores alone
          (device events around the enqueue, no host read) and (b) the whole call with its one 64-byte copy and the host
          divisions (host clock)
  host    the same function on the numpy arrays: scipy binary_erosion + two distance_transform_edt (host clock)
Medians after warm-up; the host path runs 5 times where one call takes < 2 s and 2 times otherwise (stated per row).  The
scores of the two paths are compared before anything is timed.  candidates = 2 n (d1 + d0), the min-plus evaluations of the
brute-force passes."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aide_amd._lib import lib, check
from aide_amd.ops import ptr, stream_ptr
from aide_amd.utils.metrics3d import surface_scores

SHAPES = ((256, 256, 33), (512, 512, 100))
SPACING = (1.37, 1.37, 7.7)


def ellipsoid_pair(shape):
    z, y, x = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing='ij')
    c, r = [(s - 1) / 2.0 for s in shape], [0.36 * s for s in shape]

    def ball(cz, cy, cx, k=1.0):
        return ((z - cz) / (k * r[0])) ** 2 + ((y - cy) / (k * r[1])) ** 2 + ((x - cx) / (k * r[2])) ** 2 <= 1.0
    t = ball(*c)
    p = ball(c[0] + 0.06 * shape[0], c[1] - 0.04 * shape[1], c[2] + 0.05 * shape[2]) & ~ball(c[0] + r[0], c[1], c[2], 0.4)
    return p.astype(np.uint8), t.astype(np.uint8)


def med_device(fn, reps=20, warm=3):
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


def med_host(fn, reps, warm=1):
    for _ in range(warm):
        fn()
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

    out('# surface distances: device vs host (%s)' % torch.cuda.get_device_name(0))
    out('%-12s %9s %9s %13s %12s %12s %11s %6s %9s' % ('shape', 'n_pred', 'n_target', 'candidates', 'kernels ms', 'call ms',
                                                      'host ms', 'host n', 'speed-up'))
    for shape in SHAPES:
        p, t = ellipsoid_pair(shape)
        pd, td = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
        got = surface_scores(pd, td, SPACING)
        t0 = time.perf_counter()
        ref = surface_scores(p, t, SPACING)
        one = time.perf_counter() - t0
        for k in ('n_pred', 'n_target', 'V_pred', 'V_target', 'RAVD'):
            assert got[k] == ref[k], (shape, k, got[k], ref[k])
        for k in ('ASSD', 'MSSD'):
            assert abs(got[k] - ref[k]) <= 1e-12 * abs(ref[k]), (shape, k, got[k], ref[k])
        words = torch.empty(8, device=dev, dtype=torch.int64)
        ws = torch.empty(lib.aide_surface3d_ws_bytes(pd.numel()), device=dev, dtype=torch.uint8)

        def kernels():
            check(lib.aide_surface3d_scores(ptr(pd), 1, *pd.stride(), ptr(td), 1, *td.stride(), *pd.shape, *SPACING, -1, ptr(words),
                                            None, ptr(ws), stream_ptr()), 'surface3d_scores')
        t_k = med_device(kernels)
        t_call = med_host(lambda: surface_scores(pd, td, SPACING), 20, warm=3)
        n_host = 5 if one < 2.0 else 2
        t_host = med_host(lambda: surface_scores(p, t, SPACING), n_host, warm=0)
        cand = 2.0 * p.size * (shape[0] + shape[1])
        out('%-12s %9d %9d %13.3g %12.3f %12.3f %11.1f %6d %8.0fx' % ('x'.join(map(str, shape)), got['n_pred'], got['n_target'],
                                                                      cand, t_k, t_call, t_host, n_host, t_host / t_call))
        out('%-12s RAVD %.4f %%  ASSD %.6f mm  MSSD %.6f mm (device); kernels: %.1f G candidates/s' % (
            '', got['RAVD'], got['ASSD'], got['MSSD'], cand / t_k / 1e6))
        del pd, td, ws
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
