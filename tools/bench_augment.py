"""The proposed loaders' transform chain: on the device (utils/loader_aug.py, aide_amd/csrc/augment.hip) vs PIL on the
host.  usage (GPU box): python tools/bench_augment.py [--out FILE]

Two-modal synthetic slices (synthetic.chaos_slice, u8, source size = img_size), 4 views per sample, bs 4 and 8, 256^2 and
512^2.  Device: HIP events around (a) the whole LoaderAugment call (pinned packing + upload + 2 launches, base and view
tensors written) and (b) the aide_loader_aug entry point alone on uploaded buffers (resize + emit launches); medians of
200 after 20 warm-up calls.  TB/s: float32 bytes the emit launch writes (2 modalities x 5 images x N x 3 x S^2 x 4 B)
over (b), a lower bound of the emit's own rate since (b) holds the resize launch too.  Host: the reference chain as PIL
calls (convert RGB, Resize x5, rotate x4, flip, ToTensor, Normalize per modality), single-threaded, per sample and per
batch (median of 5)."""
import argparse
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from aide_amd._lib import lib, check
from aide_amd.ops import stream_ptr
from aide_amd.synthetic import chaos_slice
from aide_amd.utils.loader_aug import LoaderAugment, draw_aug_params


def ev_median(fn, reps=200, warm=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def host_sample(planes, S, degs, flips):
    out = []
    for a in planes:
        im = Image.fromarray(a).convert('RGB')
        base = im.resize((S, S), Image.BILINEAR)
        views = [im.copy().resize((S, S), Image.BILINEAR).rotate(d, Image.BILINEAR) for d in degs]
        views = [v.transpose(Image.FLIP_LEFT_RIGHT) if f else v for v, f in zip(views, flips)]
        t = torch.from_numpy(np.array(base).transpose(2, 0, 1)).float() / 255.0
        mean = t.mean(dim=(1, 2)).unsqueeze(1).unsqueeze(2)
        std = t.std(dim=(1, 2)).unsqueeze(1).unsqueeze(2)
        out.append(t.sub(mean).div(std))
        for v in views:
            out.append((torch.from_numpy(np.array(v).transpose(2, 0, 1)).float() / 255.0).sub(mean).div(std))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.set_num_threads(1)
    dev = torch.device('cuda:0')
    lines = ['# loader transforms: device (LoaderAugment) vs host PIL chain; 2 modalities, 4 views, medians',
             '%-10s %10s %10s %10s %12s %12s %12s' % ('case', 'call_us', 'kernels_us', 'emit_TB/s', 'pil_sample_ms',
                                                     'pil_batch_ms', 'speedup')]
    for S in (256, 512):
        for N in (4, 8):
            r = np.random.RandomState(S + N)
            sl = [chaos_slice(r, S) for _ in range(N)]
            imgs = [(s[0], s[1]) for s in sl]
            p = draw_aug_params(N, 60.0, random.Random(N))
            aug = LoaderAugment(S, 60.0)
            t_call = ev_median(lambda: aug(imgs, p, device=dev))
            # the entry point alone, on buffers uploaded once: capture what the call passes
            cap = {}
            real = lib.aide_loader_aug

            class Grab(object):
                def __call__(self, *args):
                    cap['args'] = args
                    return real(*args)
            lib._fns['aide_loader_aug'] = Grab()
            try:
                keep = aug(imgs, p, device=dev)
            finally:
                lib._fns['aide_loader_aug'] = real
            args = list(cap['args'])
            # (the upload buffer and workspace the call freed: hold fresh copies for the repeated launches)
            ws = torch.empty(lib.aide_loader_aug_ws_bytes(N * 2, S), dtype=torch.uint8, device=dev)
            args[11] = ws.data_ptr()
            torch.cuda.synchronize()
            t_k = ev_median(lambda: check(real(*(args[:12] + [stream_ptr()])), 'loader_aug'))
            del keep
            emit_bytes = 2 * 5 * N * 3 * S * S * 4
            th = []
            for _ in range(5):
                t0 = time.perf_counter()
                for i in range(N):
                    host_sample(imgs[i], S, [p['degree%d' % k][i] for k in range(1, 5)],
                                [p['hflip%d' % k][i] for k in range(1, 5)])
                th.append((time.perf_counter() - t0) * 1e3)
            tb = float(np.median(th))
            lines.append('%-10s %10.1f %10.1f %10.2f %12.2f %12.2f %11.0fx' % ('bs%d_%d' % (N, S), t_call, t_k,
                         emit_bytes / (t_k * 1e-6) / 1e12, tb / N, tb, tb * 1e3 / t_call))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
