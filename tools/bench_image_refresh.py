"""Per-image pseudo-label refresh: its kernels and the whole rule (profiles/r09_image_refresh.txt).

    python tools/bench_image_refresh.py [--images 4096 32768] [--size 256] [--reps 9] [--host-images 4096]

Per K (planes of size x size):
  epilogue  `aide_image_eval_logits` over all K images in batches of 16 (as `ImageLabelBank.refresh` issues it, the forward
            excluded): bytes moved = K * HW * (8 logits + 1 score + 1 label), against the 8 TB/s of the data sheet
  select    `aide_image_refresh_select`
  update    `aide_image_bank_update` with a quarter of the images written: bytes = 2 * written * HW
  refresh   `ImageLabelBank.refresh_from_labels` + `image_dice()` (label maps on the device, forward excluded) against the same
            rule the reference's way: per image a `.cpu().numpy()` of the label map and of the target, Dice2d, on 16 host
            threads, a host sort, and a per-image copy back of the selected predictions (--host-images only: it is slow)
Device times: events around `reps` back-to-back repetitions after a warm-up, median of 5 such groups.  Same box, one process."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dev_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, nargs='+', default=[4096, 32768])
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--host-images', type=int, nargs='*', default=[4096])
    a = ap.parse_args()
    from aide_amd.inference import image_eval_logits, image_refresh_select, image_bank_update
    from aide_amd.labelbank import ImageLabelBank
    dev = torch.device('cuda:0')
    h = w = a.size
    hw = h * w
    print('per-image refresh, %dx%d planes, medians of 5 groups of %d (min .. max)' % (h, w, a.reps))
    for K in a.images:
        g = torch.Generator(device=dev).manual_seed(K)
        orig = ((torch.rand(K, h, w, device=dev, generator=g) < 0.2).to(torch.uint8) * 255)
        labels = [(torch.rand(K, h, w, device=dev, generator=g) < 0.2).to(torch.uint8) for _ in range(2)]
        logits = torch.randn(16, 2, h, w, device=dev, generator=g)
        bank = ImageLabelBank(orig, labelled=[0], form='breast')

        def epilogue():
            for i in range(0, K, 16):
                image_eval_logits(logits, orig[i:i + 16], None, i, bank._pred[0], bank._sums[0])
        med, lo, hi = dev_ms(epilogue, 1 if K > 8192 else a.reps)
        gb = K * hw * 10.0 / 1e9
        print('K %6d  epilogue  %9.3f ms (%.3f .. %.3f)  %8.1f GB/s = %4.1f %% of 8 TB/s  (%d launches of 16 images)' %
              (K, med, lo, hi, gb / med * 1e3, gb / med * 1e3 / 80.0, (K + 15) // 16))
        bank.refresh_from_labels(labels[0], labels[1], 0, 1)
        sums = bank._sums[0]
        out = (torch.empty(K, device=dev), torch.empty(K, device=dev, dtype=torch.int32), torch.empty(K, device=dev, dtype=torch.uint8))
        med, lo, hi = dev_ms(lambda: image_refresh_select(sums, None, bank.n_select, out=out), a.reps)
        print('K %6d  select    %9.3f ms (%.3f .. %.3f)' % (K, med, lo, hi))
        written = (torch.arange(K, device=dev) % 4 == 0).to(torch.uint8)
        plane = orig.clone()
        med, lo, hi = dev_ms(lambda: image_bank_update(bank._pred[0], written, 255, plane), a.reps)
        gb = 2.0 * (K // 4) * hw / 1e9
        print('K %6d  update    %9.3f ms (%.3f .. %.3f)  %8.1f GB/s of written planes (a quarter of the images)' %
              (K, med, lo, hi, gb / med * 1e3))

        def device_refresh():
            b = ImageLabelBank(orig, labelled=[0], form='breast')
            b.refresh_from_labels(labels[0], labels[1], 0, 1)
            return b, b.image_dice()

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r
        device_refresh()
        td = [wall(device_refresh) for _ in range(3)]
        print('K %6d  refresh   %9.2f ms wall (min of 3; bank construction, both networks, image_dice() included)' %
              (K, min(t for t, _ in td)))
        if K in a.host_images:
            def host_refresh():
                planes = [orig.clone(), orig.clone()]
                score = [orig, planes[0]]
                dice = [torch.zeros(K), torch.zeros(K)]
                preds = [[None] * K, [None] * K]

                def one(k):
                    for n in (0, 1):
                        p = labels[n][k].cpu().numpy().astype(np.int64)
                        t = (score[n][k].cpu().numpy() > 0).astype(np.int64)
                        u = p.sum() + t.sum()
                        dice[n][k] = 0.0 if u == 0 else 2 * np.sum(p * t) / u
                        preds[n][k] = p
                with ThreadPoolExecutor(16) as ex:
                    list(ex.map(one, range(K)))
                for n in (0, 1):
                    for k in dice[n].sort(stable=True)[1][:int(0.25 * K)].tolist():
                        if k != 0 and preds[n][k].sum() > 0:
                            planes[n][k] = torch.from_numpy((preds[n][k] * 255).astype(np.uint8)).to(dev)
                return planes, dice
            th, (planes, dice) = wall(host_refresh)
            b, d = td[-1][1]
            same = all(torch.equal(b.bank[n], planes[n]) for n in (0, 1)) and torch.equal(d, torch.stack(dice))
            print('K %6d  host rule %9.2f ms wall (per-image .cpu() copies, 16 threads): x %.1f; banks and Dice equal: %s' %
                  (K, th, th / min(t for t, _ in td), same))
        del bank, orig, labels, plane
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
