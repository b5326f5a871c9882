"""Test-time augmentation at inference: the fused path against the same ensemble composed from torch ops, and the two
kernels alone (profiles/r15_ensemble.txt).

    python tools/bench_ensemble.py [--reps 7] [--batch_size 16] [--out profiles/r15_ensemble.txt]

Workloads: FuseUNet on a 256 x 256 x 33 case and UNet on 33 slices of 320 x 320, views 'flip4' and 'd4'.  Per workload
  (a) `predict_labels(net, ..., views=...)`: aide_view_stack, one forward per chunk on the stacked views, aide_ensemble_vote;
  (b) the same ensemble from torch ops on this tree: per view flip / rot90, the forward, the inverse, softmax, then the mean
      over the views and argmax -- the same chunks of slices; its labels are compared with (a)'s;
  (c) `predict_labels(net, ...)`: the plain single forward.
(a), (b), (c) alternate inside every repetition; slices/s from the median wall time between two device synchronisations.
The kernels alone: dispatch begin-to-end times of the library's kernel timer over 50 launches each (after 5 warm-up
launches), for a flip-only and a rotated member set; effective GB/s = (bytes read + bytes written) / time."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch_size', type=int, default=16)
    ap.add_argument('--slices', type=int, default=33)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15_ensemble.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ensemble: no HIP device; nothing is measured without one')
    from aide_amd._lib import lib, check
    from aide_amd.inference import predict_labels, ensemble_vote, view_stack, view_codes, view_apply_host, view_invert_host
    from aide_amd.models_singlemodalinput import UNet
    from aide_amd.models_twomodalinputs import fuseunet
    dev = torch.device('cuda:0')
    lines = []

    def out(s=''):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    out('test-time augmentation, %s, %d slices per case, batch_size %d, %d interleaved repetitions'
        % (torch.cuda.get_device_name(0), a.slices, a.batch_size, a.reps))
    out('%-34s %12s %12s %12s %10s' % ('workload', '(a) fused', '(b) torch', '(c) single', 'labels'))
    out('%-34s %12s %12s %12s %10s' % ('', 'slices/s', 'slices/s', 'slices/s', '(a) != (b)'))
    for name, make, size, two in (('FuseUNet 256x256', lambda: fuseunet(2), 256, True), ('UNet 320x320', lambda: UNet(2), 320, False)):
        torch.manual_seed(2)
        net = make().to(dev).eval()
        g = torch.Generator().manual_seed(8)
        xs = tuple(torch.randn(a.slices, 3, size, size, generator=g).to(dev) for _ in range(2 if two else 1))
        for views in ('flip4', 'd4'):
            codes = view_codes(views, size, size)
            step = max(1, a.batch_size // len(codes))

            def fused():
                return predict_labels(net, *xs, views=views, batch_size=a.batch_size)

            def composed():
                labels = []
                with torch.no_grad():
                    for i in range(0, a.slices, step):
                        ps = []
                        for v in codes:
                            z = net(*[view_apply_host(x[i:i + step], v).contiguous() for x in xs])
                            ps.append(torch.softmax(view_invert_host(z, v), 1))
                        labels.append(torch.stack(ps).mean(0).argmax(1))
                return torch.cat(labels)

            def single():
                return predict_labels(net, *xs, batch_size=a.batch_size)

            la, lb = fused(), composed()                            # warm-up of every shape, and the two ways compared
            single()
            diff = int((la != lb).sum().item())
            res = {'a': [], 'b': [], 'c': []}
            for _ in range(a.reps):
                res['a'].append(timed(fused)[0])
                res['b'].append(timed(composed)[0])
                res['c'].append(timed(single)[0])
            rate = {k: a.slices / (np.median(v) * 1e-3) for k, v in res.items()}
            out('%-34s %12.1f %12.1f %12.1f %10s' % ('%s %s (V = %d)' % (name, views, len(codes)), rate['a'], rate['b'], rate['c'],
                                                     '%d of %d' % (diff, la.numel())))
            out('%-34s %s' % ('  median ms (min .. max)', '   '.join(
                '(%s) %.1f (%.1f .. %.1f)' % (k, np.median(res[k]), min(res[k]), max(res[k])) for k in 'abc')))

    # ---- the kernels alone -------------------------------------------------------------------------------------------------
    def kernel_us(fn, launches=50):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        check(lib.aide_ktimer_start(1 << 15, launches + 8), 'ktimer_start')
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
        n, ms, wk, mx = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        rc = lib.aide_ktimer_read(15, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(wk), ctypes.byref(mx))
        lib.aide_ktimer_stop()
        if rc < 0 or n.value != launches:
            raise RuntimeError('kernel timer: rc %d, %d launches recorded of %d' % (rc, n.value, launches))
        return ms.value * 1e3 / launches, mx.value * 1e3

    out()
    out('kernels alone (mean and max of 50 dispatches)')
    out('%-52s %10s %10s %10s' % ('kernel, shape, member set', 'mean us', 'max us', 'GB/s'))
    g = torch.Generator().manual_seed(9)
    for n, c, size in ((16, 2, 256), (16, 8, 256), (16, 2, 320)):
        for label, codes in (('flip-only (0,4,2,6)', (0, 4, 2, 6)), ('rotated (1,3,5,7)', (1, 3, 5, 7))):
            k = len(codes)
            z = torch.randn(k, n, c, size, size, generator=g).to(dev)
            members = list(z)
            for probs in (False, True):
                us, mx = kernel_us(lambda: ensemble_vote(members, codes, probs=probs))
                nbytes = 4.0 * k * n * c * size * size + 8.0 * n * size * size + (4.0 * n * c * size * size if probs else 0.0)
                out('%-52s %10.1f %10.1f %10.1f' % ('vote%s K=%d N=%d C=%d %dx%d %s' % (' +probs' if probs else '', k, n, c, size, size,
                                                                                       label), us, mx, nbytes / us * 1e-3))
    for n, size in ((16, 256), (16, 320)):
        x = torch.randn(n, 3, size, size, generator=g).to(dev)
        for label, codes in (('flip-only (0,4,2,6)', (0, 4, 2, 6)), ('rotated (1,3,5,7)', (1, 3, 5, 7)), ('d4', tuple(range(8)))):
            us, mx = kernel_us(lambda: view_stack(x, codes))
            nbytes = 4.0 * (1 + len(codes)) * n * 3 * size * size
            out('%-52s %10.1f %10.1f %10.1f' % ('view_stack V=%d N=%d C=3 %dx%d %s' % (len(codes), n, size, size, label), us, mx,
                                                nbytes / us * 1e-3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
