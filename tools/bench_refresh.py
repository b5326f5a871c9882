"""Epoch-end evaluation of the proposed loop, per case against batched (profiles/r08_refresh.txt).

    python tools/bench_refresh.py [--cases 40] [--slices 33] [--size 256] [--reps 7]

(a) the per-case way: for every case and network `predict_case(..., keep_largest=True, numpy=False)` + `case_scores`
    (five filter launches, one confusion launch and one blocking copy per case and network), the rule on the host;
(b) `PseudoLabelBank.refresh` (all slices through the network, one batched filter / sums / ranking / update per network)
    + `case_dice()`.
Two lines: the whole chain, and the post-processing alone (label maps computed beforehand, forward excluded).  (a) and (b)
alternate inside every repetition; median and min .. max of the wall time between two device synchronisations."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=int, default=40)
    ap.add_argument('--slices', type=int, default=33)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch_size', type=int, default=16)
    a = ap.parse_args()
    from aide_amd.inference import (predict_case, predict_labels, case_scores, keep_largest_connected_components,
                                    evaluate_label_maps)
    from aide_amd.labelbank import PseudoLabelBank
    from aide_amd.models_twomodalinputs import fuseunet
    from aide_amd.synthetic import chaos_batch
    dev = torch.device('cuda:0')
    K, S = a.cases, a.slices
    xi, xo, t = chaos_batch(S, a.size, seed=8)
    # K cases: the same anatomy shifted by k pixels (distinct predictions, no host time spent drawing 1320 slices)
    inphase = torch.cat([torch.roll(xi, k, 3) for k in range(K)]).to(dev)
    outphase = torch.cat([torch.roll(xo, k, 3) for k in range(K)]).to(dev)
    init = torch.cat([torch.roll(t, k, 2) for k in range(K)]).to(torch.uint8).mul_(63).to(dev)
    start = [k * S for k in range(K + 1)]
    torch.manual_seed(2)
    nets = [fuseunet(2).to(dev).eval() for _ in range(2)]
    n_select = int(0.25 * K)

    def per_case(labels=None):
        banks = [init.clone(), init.clone()]
        for n, net in enumerate(nets):
            d, preds = torch.zeros(K), []
            for k in range(K):
                lo, hi = start[k], start[k + 1]
                if labels is None:
                    pred = predict_case(net, inphase[lo:hi], outphase[lo:hi], batch_size=a.batch_size, keep_largest=True, numpy=False)
                else:
                    pred = keep_largest_connected_components(labels[n][lo:hi].permute(1, 2, 0))
                d[k] = case_scores(pred, (banks[n][lo:hi] == 63).permute(1, 2, 0))['Dice']
                preds.append(pred)
            for k in d.sort(stable=True)[1][:n_select].tolist():
                if k != 0:
                    banks[n][start[k]:start[k + 1]] = (preds[k] * 63).permute(2, 0, 1)
        return banks

    def batched(labels=None):
        bank = PseudoLabelBank(init, start, [0])
        if labels is None:
            bank.refresh(nets[0], nets[1], (inphase, outphase), 0, 1, batch_size=a.batch_size)
        else:
            bank.refresh_from_labels(labels[0], labels[1], 0, 1)
        bank.case_dice()
        return bank.bank

    def timed(fn, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(*args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    labels = [predict_labels(net, inphase, outphase, batch_size=a.batch_size) for net in nets]
    ra, rb = per_case(labels), batched(labels)                        # warm-up, and the two ways agree
    same = all(torch.equal(ra[n], rb[n]) for n in (0, 1))
    per_case(), batched()
    res = {'whole a': [], 'whole b': [], 'post a': [], 'post b': []}
    for _ in range(a.reps):
        res['whole a'].append(timed(per_case)[0])
        res['whole b'].append(timed(batched)[0])
        res['post a'].append(timed(per_case, labels)[0])
        res['post b'].append(timed(batched, labels)[0])
    print('%d FuseUNet cases of %dx%dx%d, both networks, %d interleaved repetitions; banks equal: %s' %
          (K, a.size, a.size, S, a.reps, same))
    print('(a) per case: predict_case(keep_largest) + case_scores, host rule   (b) PseudoLabelBank.refresh + case_dice')
    for key in ('whole a', 'whole b', 'post a', 'post b'):
        v = np.asarray(res[key])
        what = 'whole chain' if key.startswith('whole') else 'post-processing only'
        print('%-22s (%s)  median %9.2f ms   min %9.2f   max %9.2f' % (what, key[-1], np.median(v), v.min(), v.max()))


if __name__ == '__main__':
    main()
