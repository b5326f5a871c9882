"""Sliding-window inference: the fused path against the same pipeline composed from torch ops, and the two kernels alone
(profiles/r17_window.txt).

    python tools/bench_window.py [--reps 7] [--batch_size 16] [--out profiles/r17_window.txt]

Workload: a 33-slice case at 512 x 512, windows of 256 x 256 at stride 128 (B = 9), UNet and FuseUNet, without views and with
'flip2'.  Per workload
  (a) `predict_labels(net, ..., window=256, stride=128[, views='flip2'])`: aide_window_stack, the forwards, aide_window_blend;
  (b) the same pipeline from torch ops on this tree: per window a slice of the input, the forward (per view flip, forward,
      inverse, softmax, mean), `F.softmax`, a weighted slice-assign accumulation into [g,C,H,W], then the division and argmax
      -- the same groups of slices and the same forward batches; its labels are compared with (a)'s, and must be identical
      at every pixel where the float64 top-two gap of (b)'s probabilities exceeds 1e-5.
(a) and (b) alternate inside every repetition; slices/s from the median wall time between two device synchronisations.
The kernels alone: dispatch begin-to-end times of the library's kernel timer over 50 launches each (after 5 warm-up
launches); effective TB/s = the bytes the entry declares (window pixels inside the image read once, outputs written once) /
time."""
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
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--window', type=int, default=256)
    ap.add_argument('--stride', type=int, default=128)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r17_window.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_window: no HIP device; nothing is measured without one')
    from aide_amd._lib import lib, check
    from aide_amd.inference import predict_labels, window_grid, window_weights, window_stack, window_blend, view_codes, \
        view_apply_host, view_invert_host
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

    size, win, stride = a.size, a.window, a.stride
    sy, sx = window_grid(size, size, win, stride)
    cells = [(y0, x0) for y0 in sy for x0 in sx]
    nb = len(cells)
    gh, gw = (g.to(dev) for g in window_weights(win))
    wgt = gh[:, None] * gw[None, :]
    out('sliding-window inference, %s, %d slices of %d x %d, windows %d x %d at stride %d (B = %d), batch_size %d, %d '
        'interleaved repetitions' % (torch.cuda.get_device_name(0), a.slices, size, size, win, win, stride, nb, a.batch_size, a.reps))
    out('%-28s %12s %12s %22s' % ('workload', '(a) fused', '(b) torch', 'labels (a) != (b)'))
    out('%-28s %12s %12s %22s' % ('', 'slices/s', 'slices/s', 'all / where gap > 1e-5'))
    for name, make, two in (('UNet', lambda: UNet(2), False), ('FuseUNet', lambda: fuseunet(2), True)):
        torch.manual_seed(2)
        net = make().to(dev).eval()
        g = torch.Generator().manual_seed(8)
        xs = tuple(torch.randn(a.slices, 3, size, size, generator=g).to(dev) for _ in range(2 if two else 1))
        for views in (None, 'flip2'):
            codes = (0,) if views is None else view_codes(views, win, win)
            v = len(codes)
            group = max(1, a.batch_size // (nb * v))
            chunk = max(1, a.batch_size // v)

            def fused():
                return predict_labels(net, *xs, window=win, stride=stride, views=views, batch_size=a.batch_size)

            def composed(want_probs=False):
                labels, probs = [], []
                with torch.no_grad():
                    for i in range(0, a.slices, group):
                        gn = min(group, a.slices - i)
                        crops = [torch.cat([x[i:i + gn, :, y0:y0 + win, x0:x0 + win] for y0, x0 in cells]) for x in xs]
                        ps = []
                        for j in range(0, nb * gn, chunk):
                            part = [c[j:j + chunk] for c in crops]
                            if views is None:
                                ps.append(torch.softmax(net(*part), 1))
                            else:
                                ps.append(torch.stack([torch.softmax(view_invert_host(
                                    net(*[view_apply_host(p, code).contiguous() for p in part]), code), 1) for code in codes]).mean(0))
                        p = torch.cat(ps).view((nb, gn) + tuple(ps[0].shape[1:]))
                        acc = torch.zeros(gn, p.shape[2], size, size, device=dev)
                        den = torch.zeros(size, size, device=dev)
                        for b, (y0, x0) in enumerate(cells):
                            acc[:, :, y0:y0 + win, x0:x0 + win] += wgt * p[b]
                            den[y0:y0 + win, x0:x0 + win] += wgt
                        acc /= den
                        labels.append(acc.argmax(1))
                        if want_probs:
                            probs.append(acc)
                return (torch.cat(labels), torch.cat(probs)) if want_probs else torch.cat(labels)

            la = fused()                                            # warm-up of every shape, and the two ways compared
            lb, pb = composed(want_probs=True)
            top = pb.double().topk(2, dim=1).values
            clear = (top[:, 0] - top[:, 1]) > 1e-5
            diff, diff_clear = int((la != lb).sum().item()), int(((la != lb) & clear).sum().item())
            del pb, top
            res = {'a': [], 'b': []}
            for _ in range(a.reps):
                res['a'].append(timed(fused)[0])
                res['b'].append(timed(composed)[0])
            rate = {k: a.slices / (np.median(t) * 1e-3) for k, t in res.items()}
            out('%-28s %12.1f %12.1f %22s' % ('%s%s' % (name, '' if views is None else ' %s (V = %d)' % (views, v)), rate['a'], rate['b'],
                                             '%d / %d of %d' % (diff, diff_clear, la.numel())))
            out('%-28s %s' % ('  median ms (min .. max)', '   '.join(
                '(%s) %.1f (%.1f .. %.1f)' % (k, np.median(res[k]), min(res[k]), max(res[k])) for k in 'ab')))
            assert diff_clear == 0, '%d labels differ where the float64 gap exceeds 1e-5' % diff_clear

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
        return ms.value * 1e3 / launches, mx.value * 1e3, wk.value / launches

    out()
    out('kernels alone (mean and max of 50 dispatches; bytes as the entries declare them)')
    out('%-52s %10s %10s %10s' % ('kernel, shape', 'mean us', 'max us', 'TB/s'))
    g = torch.Generator().manual_seed(9)
    for n in (1, 4):
        x = torch.randn(n, 3, size, size, generator=g).to(dev)
        us, mx, nbytes = kernel_us(lambda: window_stack(x, win, stride))
        out('%-52s %10.1f %10.1f %10.2f' % ('window_stack B=%d N=%d C=3 %dx%d' % (nb, n, size, size), us, mx, nbytes / us * 1e-6))
        for c in (2, 8):
            z = torch.randn(nb, n, c, win, win, generator=g).to(dev)
            for probs in (False, True):
                for logits in (True, False):
                    us, mx, nbytes = kernel_us(lambda: window_blend(z, (size, size), win, stride, logits=logits, probs=probs))
                    out('%-52s %10.1f %10.1f %10.2f' % ('blend%s%s B=%d N=%d C=%d %dx%d' % (
                        ' +probs' if probs else '', '' if logits else ' (probabilities in)', nb, n, c, size, size), us, mx,
                        nbytes / us * 1e-6))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
