"""Resampling on the device vs the same result composed from torch ops on the device and vs the host statement.
usage (GPU box): python tools/bench_resample.py [--out profiles/r20_resample.txt]

The synthetic five-class volume of tools/bench_postprocess.py at 256^2 x 33 and at 512^2 x 100 ([H,W,S]), spacing 1.37 x 1.37 x 7.7
mm, resampled to 1 mm in-plane (`resampled_shape`: 351^2 x 33 and 701^2 x 100) and back.  Variants, timed in one process with device
events around the public call (workspace and result allocation included), ALTERNATING: every round times each variant once,
medians over the rounds after warm-up:
  labels up / back    resample_labels(C = 5): int64 and uint8, contiguous and as the [H,W,S] permuted view of [S,H,W] memory that
                      `predict_case` returns
  probs C = 2, 5, 8   resample_probs of [S,C,H',W'] soft-max maps on the 1 mm grid back to (S, H, W), labels only
  image               resample_image of a [S,3,H,W] modal input per slice and channel to (H', W')
  torch labels        F.one_hot -> F.interpolate(trilinear, align_corners=False) -> argmax on the device (float32: its ties
                      may fall differently; the share of equal voxels is reported)
  torch probs C = 5 / torch image    F.interpolate on the same operands
  host                the numpy float64 statement (host clock, one run; the small volume only)
Effective TB/s = compulsory bytes / time: every input element read once, every output element written once; B/vox is that per
output voxel.  Nothing here is a gate.  The device results are compared with the host statement before anything is timed."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import torch.nn.functional as F

from aide_amd.resample import resample_image, resample_labels, resample_probs, resampled_shape
from bench_morphology import alternate, host_ms
from bench_postprocess import organs, launch_split

SHAPES = ((256, 256, 33), (512, 512, 100))
SPACING = (1.37, 1.37, 7.7)
TARGET = (1.0, 1.0, 7.7)
C = 5


def torch_labels(t, e):
    onehot = F.one_hot(t, C).permute(3, 0, 1, 2).unsqueeze(0).float()
    return F.interpolate(onehot, size=e, mode='trilinear', align_corners=False)[0].argmax(0)


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
    out('# resampling %s mm -> %s mm and back vs torch ops on the device vs the host statement (%s)' % (
        ' x '.join(map(str, SPACING)), ' x '.join(map(str, TARGET)), torch.cuda.get_device_name(0)))
    out('# ms = median of 15 alternating rounds; TB/s = (input bytes + output bytes) / time, B/vox = those bytes per output voxel')
    splits = []
    for d in SHAPES:
        e, real = resampled_shape(d, SPACING, TARGET)
        h, w, s = d
        v = organs(*d, rng)
        small = v.size < 2 ** 22
        t64 = torch.from_numpy(v).to(dev)
        up64 = resample_labels(t64, e, C)
        fine = {'int64': up64.to(torch.int64), 'uint8': up64}
        coarse = {'int64': t64, 'uint8': t64.to(torch.uint8)}
        host = {}
        if small:                                 # the host runs double as the check of the device results
            box = []
            host['labels up int64'] = host_ms(lambda: box.append(resample_labels(v, e, C)))
            assert np.array_equal(up64.cpu().numpy(), box[0]), d
            host['labels back int64'] = host_ms(lambda: box.append(resample_labels(box[0], d, C)))
            assert np.array_equal(resample_labels(up64, d, C).cpu().numpy(), box[1]), d
        variants, nbytes = {}, {}
        for ty, size in (('int64', 8), ('uint8', 1)):
            for lay in ('', ' [H,W,S] view'):
                a, b = coarse[ty], fine[ty]
                if lay:
                    a, b = (x.permute(2, 0, 1).contiguous().permute(1, 2, 0) for x in (a, b))
                    assert torch.equal(resample_labels(a, e, C), up64)
                variants['labels up %s%s' % (ty, lay)] = lambda a=a: resample_labels(a, e, C)
                variants['labels back %s%s' % (ty, lay)] = lambda b=b: resample_labels(b, d, C)
                nbytes['labels up %s%s' % (ty, lay)] = (v.size * size + up64.numel(), up64.numel())
                nbytes['labels back %s%s' % (ty, lay)] = (up64.numel() * size + v.size, v.size)
        g = torch.Generator(device=dev).manual_seed(3)
        probs = {}
        for c in (2, 5, 8):
            p = probs[c] = torch.softmax(torch.randn((s, c, e[0], e[1]), device=dev, generator=g), 1)
            variants['probs C=%d' % c] = lambda p=p: resample_probs(p, (s, h, w))
            nbytes['probs C=%d' % c] = (p.numel() * 4 + v.size * 8, v.size)
        x = torch.randn((s, 3, h, w), device=dev, generator=g)
        variants['image'] = lambda: resample_image(x.reshape(-1, 1, h, w), (1,) + e[:2])
        nbytes['image'] = (4 * (x.numel() + s * 3 * e[0] * e[1]), s * 3 * e[0] * e[1])
        if small:
            p2 = probs[2][:, :, :64].contiguous()
            assert np.array_equal(resample_probs(p2, (s, 40, w)).cpu().numpy(), resample_probs(p2.cpu().numpy(), (s, 40, w)))
            x2 = x[:2].reshape(-1, 1, h, w)
            assert resample_image(x2, (1,) + e[:2]).cpu().numpy().tobytes() == resample_image(x2.cpu().numpy(), (1,) + e[:2]).tobytes()
        agree = float((torch_labels(t64, e) == up64).float().mean())
        variants['torch labels up'] = lambda: torch_labels(t64, e)
        variants['torch labels back'] = lambda: torch_labels(fine['int64'], d)
        nbytes['torch labels up'], nbytes['torch labels back'] = nbytes['labels up int64'], nbytes['labels back int64']
        p5 = probs[5].permute(1, 0, 2, 3).unsqueeze(0)
        variants['torch probs C=5'] = lambda: F.interpolate(p5, size=(s, h, w), mode='trilinear', align_corners=False)[0].argmax(0)
        nbytes['torch probs C=5'] = nbytes['probs C=5']
        variants['torch image'] = lambda: F.interpolate(x, size=e[:2], mode='bilinear', align_corners=False)
        nbytes['torch image'] = nbytes['image']
        ms = alternate(variants)
        tag = 'x'.join(map(str, d))
        out()
        out('# %s -> %s (real spacing %s); torch one_hot + trilinear + argmax equals resample_labels on %.4f %% of the voxels' % (
            tag, 'x'.join(map(str, e)), ' x '.join('%.4f' % r for r in real), 100.0 * agree))
        out('%-12s %-32s %9s %7s %6s %10s' % ('shape', 'variant', 'ms', 'B/vox', 'TB/s', 'host ms'))
        for name, val in ms.items():
            b, n = nbytes[name]
            hm = host.get(name)
            out('%-12s %-32s %9.3f %7.1f %6.2f %10s' % (tag, name, val, b / n, b / (val * 1e-3) / 1e12,
                                                      '%.1f' % hm if hm is not None else '-'))
        splits.append((tag, launch_split(lambda: resample_labels(t64, e, C)), launch_split(lambda: resample_probs(probs[5], (s, h, w))),
                       launch_split(lambda: resample_image(x.reshape(-1, 1, h, w), (1,) + e[:2]))))
        del t64, up64, fine, coarse, probs, x, p5, variants
    out()
    out('# one call, launch by launch, ms (the per-axis table, then the gather)')
    for tag, lab, prb, img in splits:
        out('%-12s labels up int64  %s' % (tag, ' '.join('%7.3f' % x for x in lab)))
        out('%-12s probs C=5        %s' % (tag, ' '.join('%7.3f' % x for x in prb)))
        out('%-12s image            %s' % (tag, ' '.join('%7.3f' % x for x in img)))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
