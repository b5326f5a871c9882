"""Per-case evaluation on the device vs the CPU (trainchaos_comparison_1case.py:233-314: predict every slice, stack to
[H,W,S], keep the largest 3-D connected component, score).  usage (GPU box): python tools/bench_eval.py [--out FILE]

(a) the filter alone: aide_amd.inference.keep_largest_connected_components on a HIP tensor (device events around the
    call: the five kernels of aide_keep_largest_cc3d) vs the same function on the numpy array (host clock), on four
    volumes per shape; bytes = the algorithm's streaming traffic, 29 B per voxel (int64 labels read once, the int32
    parent / area words written, re-read by the count, select and write passes, the uint8 mask written).
(b) the whole per-case evaluation of FuseUNet 256^2 x 33 slices (slices resident on the device): predict_case ->
    CPU filter -> Dice3d_fn, vs predict_case(keep_largest=True, numpy=False) -> case_scores (host clock around a
    synchronised end).
Medians after warm-up; the CPU filter runs 20 times where one call takes < 1 s and 3 times otherwise (stated per row)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aide_amd.inference import (keep_largest_connected_components as keep, case_scores, predict_case, predict_labels,
                                Dice3d_fn)
from aide_amd.synthetic import chaos_batch

BYTES_PER_VOXEL = 29
SHAPES = ((256, 256, 33), (256, 256, 64), (320, 320, 64), (512, 512, 100))


def realistic(h, w, s, rng):
    """synthetic CHAOS targets stacked [H,W,S] + a few hundred 1-3 voxel speckles."""
    _, _, t = chaos_batch(s, h, seed=int(rng.randint(1 << 30)), single_modal=True)
    v = t.permute(1, 2, 0).contiguous().numpy().copy()
    if w != h:
        v = v[:, :w]
    for _ in range(300):
        y, x, z = rng.randint(0, h - 2), rng.randint(0, w - 2), rng.randint(0, s)
        v[y:y + 1 + rng.randint(2), x:x + 1 + rng.randint(2), z] = 1
    return v


def serpentine(d0, d1, d2):
    v = np.zeros((d0, d1, d2), np.int64)
    for z in range(0, d0, 2):
        v[z, 0::2, :] = 1
        for y in range(0, d1 - 1, 2):
            v[z, y + 1, d2 - 1 if (y // 2) % 2 == 0 else 0] = 1
        if z + 1 < d0:
            v[z + 1, d1 - 1 if d1 % 2 == 1 else d1 - 2, 0] = 1
    return v


def med_device(fn, reps=25, warm=3):
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

    out('# per-case evaluation: device vs CPU (%s)' % torch.cuda.get_device_name(0))
    out()
    out('## (a) largest connected component alone')
    out('%-14s %-11s %9s %11s %9s %10s %12s %6s %9s' % ('shape', 'input', 'fg %', 'bytes MB', 'dev ms', 'dev GB/s',
                                                      'cpu ms', 'cpu n', 'speed-up'))
    rng = np.random.RandomState(1)
    for shape in SHAPES:
        h, w, s = shape
        vols = [('realistic', realistic(h, w, s, rng)),
                ('8-class', rng.randint(0, 8, shape).astype(np.int64)),
                ('p=0.31', (rng.rand(*shape) < 0.31).astype(np.int64)),
                ('serpentine', serpentine(*shape))]
        for name, v in vols:
            t = torch.from_numpy(v).to(dev)
            got = keep(t).cpu().numpy()
            t0 = time.perf_counter()
            ref = keep(v)
            one = time.perf_counter() - t0
            assert np.array_equal(got, ref), (shape, name)
            dms = med_device(lambda: keep(t))
            n_cpu = 20 if one < 1.0 else 3
            cms = med_host(lambda: keep(v), n_cpu, warm=0)
            mb = BYTES_PER_VOXEL * v.size / 1e6
            out('%-14s %-11s %9.1f %11.1f %9.3f %10.1f %12.1f %6d %8.0fx' % (
                'x'.join(map(str, shape)), name, 100.0 * np.count_nonzero(v) / v.size, mb, dms, mb / dms,
                cms, n_cpu, cms / dms))
            del t
    out()
    out('## (b) whole per-case evaluation, FuseUNet 256x256, 33 slices (host clock, synchronised end)')
    from aide_amd.models_twomodalinputs import fuseunet
    torch.manual_seed(2)
    net = fuseunet(2).to(dev)
    net.train()
    xin, xout, _ = chaos_batch(4, 256, seed=7)
    with torch.no_grad():
        for _ in range(2):
            net(xin.to(dev), xout.to(dev))       # running statistics that are not the initial (0, 1)
    net.eval()
    xin, xout, tgt = chaos_batch(33, 256, seed=1234)
    xin, xout = xin.to(dev), xout.to(dev)
    tgt_np = tgt.permute(1, 2, 0).contiguous().numpy()
    tgt_dev = tgt.to(dev).permute(1, 2, 0)

    def cpu_chain():
        pred = keep(predict_case(net, xin, xout))
        return float(Dice3d_fn(pred, tgt_np))

    def dev_chain():
        pred = predict_case(net, xin, xout, keep_largest=True, numpy=False)
        return float(case_scores(pred, tgt_dev)['Dice'])

    def predict_only():
        predict_labels(net, xin, xout)
        torch.cuda.synchronize()

    a, b = cpu_chain(), dev_chain()
    assert a == b or (np.isnan(a) and np.isnan(b)), (a, b)
    vol = predict_case(net, xin, xout)
    t_pred = med_host(predict_only, 25, warm=3)
    t_copy = med_host(lambda: predict_case(net, xin, xout), 25, warm=3)
    t_lcc_cpu = med_host(lambda: keep(vol), 20)
    t_cpu = med_host(cpu_chain, 20, warm=2)
    t_dev = med_host(dev_chain, 25, warm=3)
    out('prediction: fg %.1f %% of %d voxels, Dice %.6f (both chains)' % (100.0 * np.count_nonzero(vol) / vol.size,
                                                                        vol.size, a))
    out('%-58s %10s' % ('step', 'ms'))
    out('%-58s %10.3f' % ('predict_labels alone (33 slices, synchronised)', t_pred))
    out('%-58s %10.3f' % ('predict_case -> numpy int64 [H,W,S] (today)', t_copy))
    out('%-58s %10.3f' % ('CPU keep_largest_connected_components of that volume', t_lcc_cpu))
    out('%-58s %10.3f' % ('CPU chain: predict_case -> CPU filter -> Dice3d_fn', t_cpu))
    out('%-58s %10.3f' % ('device chain: predict_case(keep_largest, numpy=False) -> case_scores', t_dev))
    out('%-58s %10.2fx' % ('speed-up of the device chain', t_cpu / t_dev))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
