"""HD95 and NSD on the device vs the routes that existed before.  usage (GPU box): python tools/bench_surface_select.py
[--out FILE]

Per shape, tools/bench_surface.py's ellipsoid pair (uint8 [H,W,S], spacing 1.37 x 1.37 x 7.7 mm):
  (a) aide_surface3d_scores: the five kernels (device events around the enqueue, no host read) -- the yardstick
  (b) aide_surface3d_scores_select with percentiles=(95,), tolerances=(1.0, 2.0): its 21 kernels the same way, and the whole
      surface_scores(..., percentiles=, tolerances=) call with its one copy and the host arithmetic (host clock)
  (c) the route the documents used to recommend: surface_scores(..., distances=True), a boolean-mask gather of the
      non-negative entries of each map, torch.quantile(0.95) of each, the max, .item() (host clock)
  (d) the host path: scipy distances, np.sort-based percentiles (host clock)
with the peak device memory of (b) and (c) above what is allocated before the call (torch.cuda.max_memory_allocated).
Medians after warm-up; (d) runs 5 times where one call takes < 2 s and 2 times otherwise.  The HD95 of (b), (c) and (d) are
compared before anything is timed; (c) interpolates at numpy's position, so it is held to 1e-9 relative only."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes
import numpy as np
import torch

from aide_amd._lib import lib, check
from aide_amd.ops import ptr, stream_ptr
from aide_amd.utils.metrics3d import surface_scores
from bench_surface import SHAPES, SPACING, ellipsoid_pair, med_device, med_host

QS, TAUS = (95.0,), (1.0, 2.0)


def hd95_via_maps(pd, td):
    s = surface_scores(pd, td, SPACING, distances=True)
    v = [torch.quantile(d[d >= 0], 0.95) for d in (s['dist_pred'], s['dist_target'])]
    return torch.maximum(v[0], v[1]).item()


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = []

    def out(s=''):
        print(s, flush=True)
        lines.append(s)

    out('# HD95 + NSD: percentiles=%r tolerances=%r, spacing %r (%s)' % (QS, TAUS, SPACING, torch.cuda.get_device_name(0)))
    out('%-12s %9s %9s | %10s %10s %9s | %10s %9s | %10s %9s | %10s %6s' % (
        'shape', 'n_pred', 'n_target', '(a) 5k ms', '(b) 21k ms', '(b)-(a)', '(b) call', 'peak MiB', '(c) call', 'peak MiB',
        '(d) host', 'host n'))
    for shape in SHAPES:
        p, t = ellipsoid_pair(shape)
        pd, td = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
        got = surface_scores(pd, td, SPACING, percentiles=QS, tolerances=TAUS)
        t0 = time.perf_counter()
        ref = surface_scores(p, t, SPACING, percentiles=QS, tolerances=TAUS)
        one = time.perf_counter() - t0
        for k in ('n_pred_within', 'n_target_within'):
            assert np.array_equal(got[k], ref[k]), (shape, k, got[k], ref[k])
        for k in ('HD', 'HD_pooled', 'NSD'):
            assert abs(got[k][0] - ref[k][0]) <= 1e-12 * abs(ref[k][0]), (shape, k, got[k], ref[k])
        via = hd95_via_maps(pd, td)
        assert abs(via - got['HD'][0]) <= 1e-9 * got['HD'][0], (shape, via, got['HD'])
        n = pd.numel()
        words = torch.empty(52, device=dev, dtype=torch.int64)
        ws = torch.empty(lib.aide_surface3d_select_ws_bytes(n), device=dev, dtype=torch.uint8)
        cq, ct = (ctypes.c_double * 4)(*QS), (ctypes.c_double * 4)(*TAUS)

        def five():
            check(lib.aide_surface3d_scores(ptr(pd), 1, *pd.stride(), ptr(td), 1, *td.stride(), *pd.shape, *SPACING, -1, ptr(words),
                                            None, ptr(ws), stream_ptr()), 'surface3d_scores')

        def select():
            check(lib.aide_surface3d_scores_select(ptr(pd), 1, *pd.stride(), ptr(td), 1, *td.stride(), *pd.shape, *SPACING, -1, cq,
                                                   len(QS), ct, len(TAUS), ptr(words), None, ptr(ws), stream_ptr()), 'select')
        # alternate the two so that both see the same clocks
        t_a, t_b = [], []
        for _ in range(3):
            t_a.append(med_device(five))
            t_b.append(med_device(select))
        t_a, t_b = float(np.median(t_a)), float(np.median(t_b))
        del ws, words

        def call_b():
            return surface_scores(pd, td, SPACING, percentiles=QS, tolerances=TAUS)
        t_call_b = med_host(call_b, 20, warm=3)
        t_call_c = med_host(lambda: hd95_via_maps(pd, td), 10, warm=2)
        m_b, m_c = peak_mib(call_b), peak_mib(lambda: hd95_via_maps(pd, td))
        n_host = 5 if one < 2.0 else 2
        t_host = med_host(lambda: surface_scores(p, t, SPACING, percentiles=QS, tolerances=TAUS), n_host, warm=0)
        out('%-12s %9d %9d | %10.3f %10.3f %9.3f | %10.3f %9.1f | %10.3f %9.1f | %10.1f %6d' % (
            'x'.join(map(str, shape)), got['n_pred'], got['n_target'], t_a, t_b, t_b - t_a, t_call_b, m_b, t_call_c, m_c, t_host,
            n_host))
        out('%-12s HD95 %.6f mm  HD95 pooled %.6f mm  NSD@1mm %.6f  NSD@2mm %.6f (device)' % (
            '', got['HD'][0], got['HD_pooled'][0], got['NSD'][0], got['NSD'][1]))
        del pd, td
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
