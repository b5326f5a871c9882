"""Writes tests/golden/g30_lane_schedule.json: where the two-lane forward pass of the engine's plans launches, forks, joins,
records and waits.

    python tools/gen_golden_lane_schedule.py --commit $(git rev-parse HEAD)

Needs a GPU only because a Plan owns streams and events; it launches nothing.  For every plan of PLANS it replaces ops.order,
ops.record, ops.wait, ops.maxpool2x2_fwd and Plan._forward_op by loggers (the stream of a launch is what ops.use_stream left in
ops.stream_ptr()), marks convs[4] as the gate conv, calls plan._forward_impl(inputs, out, None, None) and keeps the ordered log:

    ["op", i, role]          the launch group of step i (a whole op, or one half of a split pooling) on that stream
    ["order", from, to]      work on `to` from now on waits for the work on `from` so far
    ["record", i, role]      step i's event (ev_b) recorded on that stream
    ["wait", i, role]        that stream waits for step i's event

Streams are roles, "main" (the caller's stream) or "lane" (plan.lane_b), never pointers.  `fused_split_pools` lists the split
pooling steps (lane_split) whose halves their producers' BatchNorm kernels write (fwd_fused): they launch no pooling.  All six
names exist in every tree since f2a397a, so the same script runs on an older commit: the committed fixture states the commit it
was generated on, and tests/test_lane_schedule_host.py holds engine.lane_schedule to it on the host (entries(): the mapping
from lane_schedule's actions to these log entries)."""
import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'g30_lane_schedule.json')
TWO_MODAL = ('fuseunet', 'fuseunetsa')
LANES = ((False, False), (True, False), (True, True))          # (dual_fwd, free_lane)


def spec(model, n, size, training, groups, dual_fwd, free_lane):
    return dict(model=model, n=n, h=size, w=size, training=training, groups=groups, dual_fwd=dual_fwd, free_lane=free_lane)


# fuseunet: the training, the eval and the stacked plan, at 64 x 64 and at 256 x 256 (where fwd_fused fires), under every lane
# setting; fuseunetsa and UNet have no lane-1 ops: nothing but op entries
PLANS = [spec('fuseunet', n, size, training, groups, dual, free)
         for size in (64, 256) for n, training, groups in ((2, True, 1), (1, False, 1), (6, True, 3)) for dual, free in LANES]
PLANS += [spec(m, 2, 64, True, 1, True, True) for m in ('fuseunetsa', 'UNet')]


def make_net(sp, dev=None):
    from aide_amd import models_twomodalinputs, models_singlemodalinput
    torch.manual_seed(0)
    net = getattr(models_twomodalinputs if sp['model'] in TWO_MODAL else models_singlemodalinput, sp['model'])(2)
    if dev is not None:
        net = net.to(dev)
    net.engine.config.dual_fwd, net.engine.config.free_lane = sp['dual_fwd'], sp['free_lane']
    net.train(sp['training'])
    return net


def entries(action, fused_split_pools=()):
    """the log entries one action of engine.lane_schedule stands for: exactly one, except none for ('gate',) -- the wait for the
    filter packs is a torch call on the caller's stream, not one of the logged names -- and none for a 'pool_half' of a step in
    fused_split_pools"""
    role = ('main', 'lane')
    kind = action[0]
    if kind == 'gate' or (kind == 'pool_half' and action[1] in fused_split_pools):
        return []
    return [{'op': lambda: ['op', action[1], role[action[2]]], 'pool_half': lambda: ['op', action[1], role[action[2]]],
             'fork': lambda: ['order', 'main', 'lane'], 'join': lambda: ['order', 'lane', 'main'],
             'record': lambda: ['record', action[1], 'lane'], 'wait': lambda: ['wait', action[1], 'main']}[kind]()]


def read_plan(sp, dev):
    from aide_amd import ops
    from aide_amd.engine import Plan
    net = make_net(sp, dev)
    nin = 2 if sp['model'] in TWO_MODAL else 1
    inputs = [torch.empty(sp['n'], 3, sp['h'], sp['w'], device=dev) for _ in range(nin)]
    out = torch.empty(sp['n'], 2, sp['h'], sp['w'], device=dev)
    plan = net.engine.plan_for(inputs, sp['groups'])
    steps = plan.steps
    lane_ptr = plan.lane_b.cuda_stream if plan.lane_b is not None else None
    role = lambda s: 'lane' if (lane_ptr is not None and (getattr(s, 'value', s) or 0) == lane_ptr) else 'main'
    event = {id(st['ev_b']): i for i, st in enumerate(steps) if st.get('ev_b') is not None}
    half = {}                            # data pointer of a split pooling's destination half -> its step
    for i, st in enumerate(steps):
        c = st.get('lane_split') if st['kind'] == 'pool' else None
        if c:
            for t in (st['dst'].slice(0, c), st['dst'].slice(c, st['dst'].C - c)):
                half[plan.view(t).data_ptr()] = i
    log = []

    def forward_op(self, st, inputs_, out_, bn_ws, sk_ws):
        r = role(ops.stream_ptr())
        assert (bn_ws is plan.bn_ws and sk_ws is plan.sk_ws) if r == 'main' else (bn_ws is plan.bn_ws_b and sk_ws is plan.sk_ws_b)
        log.append(['op', [i for i, s in enumerate(steps) if s is st][0], r])

    saved = (ops.order, ops.record, ops.wait, ops.maxpool2x2_fwd, Plan._forward_op)
    ops.order = lambda ev, src, dst: log.append(['order', role(src), role(dst)])
    ops.record = lambda ev, src: log.append(['record', event[id(ev)], role(src)])
    ops.wait = lambda dst, ev: log.append(['wait', event[id(ev)], role(dst)])
    ops.maxpool2x2_fwd = lambda x, y: log.append(['op', half[y.data_ptr()], role(ops.stream_ptr())])
    Plan._forward_op = forward_op
    try:
        plan._gate_conv = [st for st in steps if st['kind'] == 'conv'][4]
        plan._coef_ok = True             # (eval: the coefficient folds are launches of their own, before the first step)
        plan._forward_impl(inputs, out, None, None)
    finally:
        ops.order, ops.record, ops.wait, ops.maxpool2x2_fwd, Plan._forward_op = saved
    fused = [i for i, st in enumerate(steps) if st['kind'] == 'pool' and st.get('lane_split') and st.get('fwd_fused')]
    return dict(spec=sp, nsteps=len(steps), fused_split_pools=fused, log=log)


def check_not_vacuous(plans):
    """a plan that pools in halves, one whose halves are written by their producers, and one without any synchronisation"""
    halves = lambda p, i: [e[2] for e in p['log'] if e[0] == 'op' and e[1] == i]
    split = [p for p in plans if any(e[0] == 'record' and halves(p, e[1]) == ['lane', 'main'] for e in p['log'])]
    fused = [p for p in plans if any(e[0] == 'record' and e[1] in p['fused_split_pools'] and not halves(p, e[1]) for e in p['log'])]
    plain = [p for p in plans if all(e[0] == 'op' for e in p['log'])]
    assert split and fused and plain, (len(split), len(fused), len(plain))
    for p in plans:                      # every step launches (a split pooling twice, or not at all)
        ops_ = [e[1] for e in p['log'] if e[0] == 'op']
        assert sorted(set(ops_) | set(p['fused_split_pools'])) == list(range(p['nsteps'])), p['spec']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit this tree is (stated in the fixture)')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    plans = [read_plan(sp, dev) for sp in PLANS]
    check_not_vacuous(plans)
    with open(args.out, 'w') as f:
        f.write('{"commit": %s,\n "plans": [\n' % json.dumps(args.commit))
        f.write(',\n'.join('  ' + json.dumps(p, separators=(',', ':')) for p in plans))
        f.write('\n ]}\n')
    with open(args.out) as f:
        assert json.load(f)['plans'] == plans
    print('%s: %d plans, %d entries, %d bytes' % (args.out, len(plans), sum(len(p['log']) for p in plans),
                                                  os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
