"""Writes tests/golden/g27_launch_trace.json: the launch sequences of four fuseunet plans, as their launch tapes recorded them,
or (--set 256) tests/golden/g29_launch_trace_256.json: those of the training and the stacked plan at 256x256.

    python tools/gen_golden_launch_trace.py --commit $(git rev-parse HEAD) [--set 256]

Needs a GPU.  Every plan of PLANS runs one forward and, where it trains ungrouped, one backward through CEMDiceLoss, with
replay on and fixed seeds; the recorded tapes (plan._tape_f / plan._tape_b) are dumped as [entry-point name, [every
non-pointer argument]] -- pointers, stream and queue handles differ from run to run and are dropped -- and Python callbacks
as ["py", tag].  `packs` is the (n, total_blocks) of every kernel family's filter-pack table of the first-four-convs launch
and of the side-stream launch (plan._pack_tabs; the pack launches run before the tape starts).  The committed fixture is
generated on the commit it names; tests/test_gpu_launch_trace.py regenerates the dumps with trace_all() and wants them equal.

The traces must hold every 3x3-conv LAUNCH entry point profiles/r05_abi_coverage.md lists as reached (entries that take a
stream; the pack launches are covered by `packs`): a plan that misses one at 128x128 would move to 256x256.

The 256x256 set exists for the lazy BatchNorm paths: conv-epilogue statistics, their precondition, first appear at that size for
these batches.  Its traces must hold aide_bn_finalize_groups, the training trace also the head's BatchNorm-applying launches."""
import argparse
import ctypes
import json
import os
import re
import sys

sys.dont_write_bytecode = True
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aide_amd._lib import lib  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'g27_launch_trace.json')
# name -> (n, size, training, precision, groups)
PLANS = dict(train_fp32=(2, 128, True, 'fp32', 1), train_bf16=(2, 128, True, 'bf16', 1), eval_fp32=(1, 128, False, 'fp32', 1),
             stacked_fp32=(6, 128, True, 'fp32', 3))
PLANS_256 = dict(train_fp32_256=(2, 256, True, 'fp32', 1), stacked_fp32_256=(6, 256, True, 'fp32', 3))
SETS = {'128': (PLANS, OUT, 'every plan at 128x128'),
        '256': (PLANS_256, os.path.join(ROOT, 'tests', 'golden', 'g29_launch_trace_256.json'), 'every plan at 256x256')}
PACK_MODES = (0, 2, 4, 16)           # order of the per-family tables where a tree keeps them as a tuple


def dump_tape(tape):
    out = []
    for cfn, cargs, rc, name in tape.calls:
        if cfn is None:
            out.append(['py', rc])
        else:
            out.append([name, [a.value for a, t in zip(cargs, lib.protos[name][1]) if t is not ctypes.c_void_p]])
    return out


def dump_packs(plan):
    (first, rest, _gate), = plan._pack_tabs.values()
    out = {}
    for tag, tabs in (('first', first), ('rest', rest)):
        items = [] if tabs is None else tabs.items() if isinstance(tabs, dict) else zip(PACK_MODES, tabs)
        out[tag] = {str(m): [t[1], t[2]] for m, t in items if t is not None}
    return out


def trace(n, size, training, precision, groups, dev):
    from aide_amd.models_twomodalinputs import fuseunet
    from aide_amd import utils as U
    torch.manual_seed(2)
    net = fuseunet(2).to(dev)
    net.engine.precision = precision
    net.train(training)
    g = torch.Generator().manual_seed(1234)
    m = n // groups
    x1, x2 = (torch.randn(m, 3, size, size, generator=g).to(dev) for _ in range(2))
    t = (torch.rand(m, size, size, generator=g) > 0.7).long().to(dev)
    w = torch.tensor([1.0, 1.0])
    if groups > 1:
        net.engine.run_groups([(x1, x2)] * groups)
    elif training:
        U.CEMDiceLoss(cediceweight=w, ceclassweight=w, diceclassweight=w)(net(x1, x2), t).backward()
    else:
        with torch.no_grad():
            net(x1, x2)
    torch.cuda.synchronize()
    plan, = net.engine.plans.values()
    out = dict(forward=dump_tape(plan._tape_f), packs=dump_packs(plan))
    if training and groups == 1:
        out['backward'] = dump_tape(plan._tape_b)
    return out


def trace_all(dev, plans=PLANS):
    return {name: trace(*(args + (dev,))) for name, args in plans.items()}


def names(tr):
    return {c[0] for k in ('forward', 'backward') for c in tr.get(k, ())}


def reached_conv_launches():
    md = open(os.path.join(ROOT, 'profiles', 'r05_abi_coverage.md')).read().split('Reached', 1)[1]
    names = re.findall(r'`(aide_conv3x3_\w+)`', md)
    header = open(os.path.join(ROOT, 'include', 'aide_hip.h')).read()
    launches = sorted(nm for nm in names if 'pack' not in nm and re.search(r'\b%s\s*\([^;]*aide_stream_t' % nm, header))
    assert len(launches) >= 8, launches          # igemm, wino, wino4, bf16 and their four weight gradients
    return launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit this tree is (stated in the fixture)')
    ap.add_argument('--set', default='128', choices=sorted(SETS), help='which plan set (and fixture) to write')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    plans, out, sizes = SETS[args.set]
    args.out = args.out or out
    traces = trace_all(torch.device('cuda:0'), plans)
    if args.set == '128':
        seen = set().union(*(names(tr) for tr in traces.values()))
        missing = [nm for nm in reached_conv_launches() if nm not in seen]
        assert not missing, 'conv launch entry points no trace holds: %s' % missing
    else:                                                             # the lazy paths fire
        for name, tr in traces.items():
            assert 'aide_bn_finalize_groups' in names(tr), name
        assert names(traces['train_fp32_256']) >= {'aide_head1x1_fwd_bn', 'aide_head1x1_wgrad_bn'}
    with open(args.out, 'w') as f:
        f.write('{"commit": %s,\n "sizes": %s,\n "plans": {\n' % (json.dumps(args.commit), json.dumps(sizes)))
        body = []
        for name, tr in traces.items():
            parts = ['   "packs": %s' % json.dumps(tr['packs'], sort_keys=True)]
            for k in ('forward', 'backward'):
                if k in tr:
                    parts.append('   "%s": [\n%s]' % (k, ',\n'.join('    ' + json.dumps(c) for c in tr[k])))
            body.append('  "%s": {\n%s}' % (name, ',\n'.join(parts)))
        f.write(',\n'.join(body) + '\n }}\n')
    print('%s: %s' % (args.out, ', '.join('%s %d+%d' % (k, len(v['forward']), len(v.get('backward', ())))
                                          for k, v in traces.items())))


if __name__ == '__main__':
    main()
