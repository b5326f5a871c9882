"""Writes tests/golden/g31_backward_schedule.json: which stream every launch, fork, hand-over, slab-reduce flush and join of the
backward pass of the engine's plans goes to, and where the per-step callback of a gradient reducer runs.

    python tools/gen_golden_backward_schedule.py --commit $(git rev-parse HEAD)

Needs a GPU.  Every plan of PLANS runs one forward and one backward under a non-default current stream (so that "main" is not the
null handle) with an `after_backward_op` that notes the step it was called for and the length of the recording tape at that
moment.  The recorded backward tape (plan._tape_b.calls) holds every C call with its ctypes arguments, stream handles included,
and the callback as a `py` entry; per entry the log keeps

    [name, role, ...]     the entry point (as an index into `names`) and the role, "main" (the caller's stream) or "side"
                          (plan.side, the weight-gradient stream), of every pointer argument equal to one of the two handles
    ["after", i]          the callback of step i

No pointers and no scalars: fixtures g27 / g29 hold the scalars.  Only names every tree since 7444a6f has are used, so the same
script runs on an older commit: the committed fixture states the commit it was generated on.  tests/test_backward_schedule_host.py
holds engine.backward_schedule to it on the host through entries(), the mapping from the schedule's actions to these log
entries; tests/test_gpu_launch_trace.py regenerates the 64 x 64 logs with read_plan() and wants them equal.

entries() names a launch by canonical(): which of the 3x3-conv kernel families runs a weight or data gradient is select_conv's
choice (fixture g26, and by exact name g27 / g29), not the schedule's, so the families' entry points collapse to
aide_conv3x3_wgrad / aide_conv3x3, and a `_mixed` storage variant to its plain name."""
import argparse
import ctypes
import json
import os
import sys

sys.dont_write_bytecode = True
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'g31_backward_schedule.json')
TWO_MODAL = ('fuseunet', 'fuseunetsa', 'fuseunetsaseparate')
FLUSH = 'aide_wgrad_queue_flush'


def spec(model, size=64, precision='fp32', overlap=True, learned=False, **config):
    return dict(model=model, learned=learned, n=2, h=size, w=size, precision=precision, overlap=overlap, config=config)


# 64 x 64: the smallest planes at which every level of the U-Nets exists.  fuseunet under every setting of the schedule's own
# switches, bf16 (no reduce queue), 256 x 256 (head_lazy, pool_fuse, fold_dgrad and the conv-epilogue statistics fire only
# there); UNet (the single-encoder tail, wg_target), fuseunetsa (the attention op), the ConvTranspose form
PLANS = [spec('fuseunet'), spec('fuseunet', tail_wgrad_main=False), spec('fuseunet', handover_on_kernel=False),
         spec('fuseunet', overlap=False), spec('fuseunet', precision='bf16'), spec('fuseunet', size=256),
         spec('UNet'), spec('fuseunetsa'), spec('UNet', learned=True)]


def booleans(sp, cfg):
    """(side, tail_main, on_kernel, batched) of engine.backward_schedule for a plan of PLANS (no profiler attached)"""
    return sp['overlap'], cfg.tail_wgrad_main, cfg.handover_on_kernel, sp['precision'] != 'bf16'


def make_net(sp, dev=None):
    from aide_amd import models_twomodalinputs, models_singlemodalinput
    torch.manual_seed(0)
    mod = models_twomodalinputs if sp['model'] in TWO_MODAL else models_singlemodalinput
    net = getattr(mod, sp['model'])(2, **(dict(learned_bilinear=True) if sp['learned'] else {}))
    if dev is not None:
        net = net.to(dev)
    net.engine.precision = sp['precision']
    for k, v in sp['config'].items():
        setattr(net.engine.config, k, v)
    net.train()
    return net


def canonical(name):
    if name.startswith('aide_conv3x3_wgrad'):
        return 'aide_conv3x3_wgrad'
    if name.startswith('aide_conv3x3_'):
        return 'aide_conv3x3'
    return name[:-len('_mixed')] if name.endswith('_mixed') else name


def launches(log):
    """a log with canonical() names, without the host-side queries of the library a tape also holds (entries no stream takes)"""
    return [e if e[0] == 'after' else [canonical(e[0])] + e[1:] for e in log if len(e) > 1]


BN_BWD = dict(grad='aide_bn_relu_bwd', pool='aide_bn_relu_bwd_pool', head='aide_bn_relu_bwd_head', slabs='aide_bn_relu_bwd_slabs')
SA_BWD = ('aide_sa_gate_bwd', 'aide_pwconv_wgrad', 'aide_pwconv_dgrad', 'aide_dconv3x3_small_wgrad', 'aide_dconv3x3_small',
          'aide_dconv3x3_small_wgrad', 'aide_dconv3x3_small', 'aide_pwconv_wgrad', 'aide_pwconv_dgrad')
WHOLE = dict(pool=('aide_maxpool2x2_bwd',), up=('aide_upsample2x_bilinear_bwd',), sa=SA_BWD)


def entries(action, steps):
    """the log entries one action of engine.backward_schedule(steps, ...) stands for, names as canonical() gives them: one per
    action, except none for ('begin', i), nine for the attention op, and for ('end', i) the callback -- which, where the slab
    reduces run batched, the executor runs behind a later flush (the log then holds it there, in the same order)"""
    role = ('main', 'side')
    kind = action[0]
    st = steps[action[1]] if len(action) > 1 else None
    if kind == 'begin':
        return []
    if kind == 'end':
        return [['after', action[1]]]
    if kind in ('fork', 'order'):
        return [['aide_stream_order', 'main', 'side']]
    if kind == 'join':
        return [['aide_stream_order', 'side', 'main']]
    if kind == 'wait':
        return [['aide_stream_wait_event', 'side']]
    if kind == 'flush':
        return [[FLUSH, role[action[2]]]]
    if kind == 'fill':
        return [['aide_fill_zero', 'main']]
    if kind == 'bn':
        return [[BN_BWD[action[2]], 'main']]
    if kind == 'wgrad':
        return [['aide_conv3x3_wgrad' if st['kind'] == 'conv' else 'aide_convT2x2_wgrad', role[action[2]]]]
    if kind == 'dgrad':
        return [['aide_conv3x3' if st['kind'] == 'conv' else 'aide_convT2x2_dgrad', 'main']]
    if kind == 'head':
        lazy = action[3] == 'wgrad' and st.get('lazy_prod') is not None
        return [['aide_head1x1_wgrad_bn' if lazy else 'aide_head1x1_bwd', role[action[2]]]]
    assert kind == 'op', action
    return [[nm, 'main'] for nm in WHOLE[st['kind']]]


def read_plan(sp, dev):
    """-> dict(spec, nsteps, log) with full entry-point names in the log"""
    from aide_amd import _lib
    net = make_net(sp, dev)
    eng = net.engine
    g = torch.Generator().manual_seed(1234)
    inputs = [torch.randn(sp['n'], 3, sp['h'], sp['w'], generator=g).to(dev) for _ in range(2 if sp['model'] in TWO_MODAL else 1)]
    notes = []                           # (step dict, length of the recording tape when its callback ran)
    eng.after_backward_op = lambda st: notes.append((st, len(_lib.TAPE[0].calls)))
    main = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(main):
        out = net(*inputs)
        plan, = eng.plans.values()
        plan.overlap = sp['overlap']
        out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    index = {id(st): i for i, st in enumerate(plan.steps)}
    after = {length - 1: index[id(st)] for st, length in notes}       # (the `py` entry is recorded right before the callback runs)
    handles = {main.cuda_stream: 'main', plan.side.cuda_stream: 'side'}
    assert len(handles) == 2 and 0 not in handles and len(after) == len(notes) == len(plan.steps)
    log = []
    for k, (cfn, cargs, rc, name) in enumerate(plan._tape_b.calls):
        if cfn is None:
            log.append(['after', after[k]])
        else:
            log.append([name] + [handles[a.value] for a, t in zip(cargs, _lib.lib.protos[name][1])
                                 if t is ctypes.c_void_p and a.value in handles])
    return dict(spec=sp, nsteps=len(plan.steps), log=log)


def check_not_vacuous(plans):
    """some plan shows each of: a hand-over by wait, one by order, the tail weight gradient on main, a flush on side, a flush on
    main, a head split across the streams, a slab-fed BatchNorm backward, callbacks deferred behind a flush"""
    def some(pred):
        return [p for p in plans if pred(launches(p['log']))]
    sided = lambda log: any('side' in e[1:] for e in log)
    wgrads = lambda log: [e for e in log if e[0] in ('aide_conv3x3_wgrad', 'aide_convT2x2_wgrad')]
    shown = dict(
        wait=some(lambda log: ['aide_stream_wait_event', 'side'] in log),
        order=some(lambda log: ['aide_stream_order', 'main', 'side'] in log[1:]),
        tail=some(lambda log: sided(log) and wgrads(log)[-1][1] == 'main' and all(e[1] == 'side' for e in wgrads(log)[:-1])),
        flush_side=some(lambda log: [FLUSH, 'side'] in log),
        flush_main=some(lambda log: [FLUSH, 'main'] in log),
        head_split=some(lambda log: any(e[0].startswith('aide_head1x1_') and e[1] == 'side' for e in log)),
        slabs=some(lambda log: ['aide_bn_relu_bwd_slabs', 'main'] in log),
        deferred=some(lambda log: any(a[0] == FLUSH and b[0] == c[0] == 'after' for a, b, c in zip(log, log[1:], log[2:]))))
    assert all(shown.values()), {k: len(v) for k, v in shown.items()}
    for p in plans:                      # every step's callback runs once, in reversed graph order
        assert [e[1] for e in p['log'] if e[0] == 'after'] == list(reversed(range(p['nsteps']))), p['spec']


def unpack(fixture):
    """the loaded fixture -> plans with full entry-point names in their logs (as read_plan gives them)"""
    return [dict(p, log=[e if e[0] == 'after' else [fixture['names'][e[0]]] + e[1:] for e in p['log']]) for p in fixture['plans']]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit this tree is (stated in the fixture)')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    plans = [read_plan(sp, dev) for sp in PLANS]
    check_not_vacuous(plans)
    names = sorted({e[0] for p in plans for e in p['log'] if e[0] != 'after'})
    packed = [dict(p, log=[e if e[0] == 'after' else [names.index(e[0])] + e[1:] for e in p['log']]) for p in plans]
    with open(args.out, 'w') as f:
        f.write('{"commit": %s,\n "names": %s,\n "plans": [\n' % (json.dumps(args.commit), json.dumps(names)))
        f.write(',\n'.join('  ' + json.dumps(p, separators=(',', ':')) for p in packed))
        f.write('\n ]}\n')
    with open(args.out) as f:
        assert unpack(json.load(f)) == plans
    print('%s: %d plans, %d entries, %d bytes' % (args.out, len(plans), sum(len(p['log']) for p in plans),
                                                  os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
