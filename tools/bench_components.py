"""Labelled components and lesion-wise counts on the device vs the component filter that does the same labelling work and vs
the host statements.
usage (GPU box): python tools/bench_components.py [--out profiles/r18_components.txt]

The synthetic five-class volumes of tools/bench_postprocess.py (same generator, same seed) at 256^2 x 33 and at 512^2 x 100; the
pair for the lesion counts is the volume as target and the volume moved by (1, 1, 0) voxels as pred.  Timed in one process:
  keep         aide_amd.inference.keep_components(volume, top_k=None, num_classes=5) on the HIP tensor (device events around
               the call: the memset, the three labelling kernels, one select pass, write): the yardstick
  label        label_components(volume, 5): the three labelling kernels, flag, scan, rank, write
  label+props  label_components(volume, 5, props=True): the memset of the table and the same seven launches
  lesion       lesion_counts(pred, target, 5, 0.5): per volume the three labelling kernels, cover, reduce; against TWO keep calls
  scores       lesion_scores(...): lesion and the one copy of the table to the host
  host         the numpy paths of label_components(props=True) and lesion_scores (scipy.ndimage.label; host clock)
Medians after warm-up.  Nothing here is a gate.  Under the table the launches of one call each are timed one by one with the
library's kernel timer (begin / end of every dispatch), so that the file says where the time goes.  The device results are
compared with the host's before anything is timed."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aide_amd.inference import keep_components, label_components, lesion_counts, lesion_scores
from bench_postprocess import organs, med_device, med_host, launch_split, SHAPES, C

LABEL_LAUNCHES = ('local', 'border', 'count', 'flag', 'scan', 'rank', 'write')
LESION_LAUNCHES = ('local', 'border', 'count', 'cover', 'reduce') * 2


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
    out('# labelled components and lesion-wise counts (C = %d) vs keep_components(top_k=None) vs the host paths (%s)' % (
        C, torch.cuda.get_device_name(0)))
    out('%-12s %7s %8s | %8s %9s %7s %12s %7s | %10s %7s %10s | %10s %11s' % (
        'shape', 'blobs', 'detected', 'keep ms', 'label ms', 'ratio', 'l+props ms', 'ratio', 'lesion ms', '/2 keep',
        'scores ms', 'host label', 'host scores'))
    for shape in SHAPES:
        v = organs(*shape, rng)
        p = np.zeros_like(v)
        p[1:, 1:, :] = v[:-1, :-1, :]
        t, tp = torch.from_numpy(v).to(dev), torch.from_numpy(p).to(dev)
        want = label_components(v, C, props=True)
        got = label_components(t, C, props=True)
        for a, b in zip(got, want):
            assert np.array_equal(a.cpu().numpy(), b), shape
        want_table = lesion_counts(p, v, C, 0.5)
        assert np.array_equal(lesion_counts(tp, t, C, 0.5).cpu().numpy(), want_table), shape
        t_keep = med_device(lambda: keep_components(t, None, 1, C))
        t_label = med_device(lambda: label_components(t, C))
        t_props = med_device(lambda: label_components(t, C, props=True))
        t_lesion = med_device(lambda: lesion_counts(tp, t, C, 0.5))
        t_scores = med_device(lambda: lesion_scores(tp, t, C, 0.5))
        n_host = 5 if v.size < 10 ** 7 else 2
        h_label = med_host(lambda: label_components(v, C, props=True), n_host)
        h_scores = med_host(lambda: lesion_scores(p, v, C, 0.5), n_host)
        out('%-12s %7d %8s | %8.3f %9.3f %7.2f %12.3f %7.2f | %10.3f %7.2f %10.3f | %10.1f %11.1f' % (
            'x'.join(map(str, shape)), int(want[1][0]), '%d/%d' % (want_table[:, 1].sum(), want_table[:, 0].sum()), t_keep, t_label,
            t_label / t_keep, t_props, t_props / t_keep, t_lesion, t_lesion / (2 * t_keep), t_scores, h_label, h_scores))
        splits.append((shape, launch_split(lambda: keep_components(t, None, 1, C)), launch_split(lambda: label_components(t, C)),
                       launch_split(lambda: label_components(t, C, props=True)),
                       launch_split(lambda: lesion_counts(tp, t, C, 0.5)), t_label / t_keep))
        del t, tp
    out()
    out('# one call, launch by launch, ms (keep: local, border, count, select, write; label: %s;' % ', '.join(LABEL_LAUNCHES))
    out('# lesion: local, border, count, cover, reduce on the target, then the same on pred)')
    for shape, keep, label, props, lesion, ratio in splits:
        tag = 'x'.join(map(str, shape))
        out('%-12s keep         %s' % (tag, ' '.join('%7.3f' % x for x in keep)))
        out('%-12s label        %s' % (tag, ' '.join('%7.3f' % x for x in label)))
        out('%-12s label+props  %s' % (tag, ' '.join('%7.3f' % x for x in props)))
        out('%-12s lesion       %s' % (tag, ' '.join('%7.3f' % x for x in lesion)))
        if ratio > 2.0 and len(label) == len(LABEL_LAUNCHES):
            out('%-12s label takes %.2f times keep_components: of its four own launches the %s launch takes the most time' % (
                tag, ratio, LABEL_LAUNCHES[3 + int(np.argmax(label[3:]))]))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
