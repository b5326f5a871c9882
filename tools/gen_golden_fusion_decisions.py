"""Writes tests/golden/g28_fusion_decisions.json: the fusion, storage and backward-write decisions of the engine's plans.

    python tools/gen_golden_fusion_decisions.py --commit $(git rev-parse HEAD)

Needs a GPU (plans own device buffers); launches nothing beyond what building a plan and plan._prepare_backward() do.  For
every plan of PLANS it reads, for every step, the decisions KEYS names from the plan's step dicts -- step dicts as indices into
plan.steps, tensors as [c0, C] within their root -- and for every graph root whether the activation / gradient buffer is stored
as bf16, and plan.lazy_bn.  Only what every tree since fa92599 stores is read, so the same script runs on an older commit: the
committed fixture states the commit it was generated on, and tests/test_fusion_decisions_host.py holds engine.select_fusions
to it on the host.  The backward-side keys are read only from plans that can run a backward (training, groups == 1), after
plan._prepare_backward(); elsewhere they are null / false.

The file is written packed, one line per plan (pack() / unpack(): lossless): `kinds` holds the step kinds once per model,
`defaults` the value of every key where no decision fired, a plan's `steps` only {step index: {key: value}} that differ from
it, its `roots` [number of roots, indices stored bf16 as activation, ... as gradient]."""
import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'g28_fusion_decisions.json')
KEYS = ('kind', 'lazy_to', 'tab_c0', 'head_lazy', 'lazy_prod', 'pool_out', 'fwd_fused',
        'src_grad', 'fold_dgrad', 'pool_fuse', 'bwd_fused', 'head_fuse', 'dgrad_fused')
TWO_MODAL = ('fuseunet', 'fuseunetsa', 'fuseunetsaseparate')
MODELS = TWO_MODAL + ('UNet', 'UNetsa')
SWITCHES = ('lazy_bn', 'lazy_head', 'fuse_head_bwd', 'fuse_pool_bwd', 'fuse_pool_fwd', 'grouped_bn',
            'store_bf16', 'store_a_bf16', 'store_g_bf16')


def spec(model, n, h, w, training, precision, groups=1, **config):
    return dict(model=model, n=n, h=h, w=w, training=training, precision=precision, groups=groups, config=config)


def modes(model, h, w):
    """training fp32, training bf16, eval fp32, stacked fp32 (+ stacked bf16 for fuseunet)"""
    out = [spec(model, 2, h, w, True, 'fp32'), spec(model, 2, h, w, True, 'bf16'), spec(model, 2, h, w, False, 'fp32'),
           spec(model, 6, h, w, True, 'fp32', groups=3)]
    if model == 'fuseunet':
        out.append(spec(model, 6, h, w, True, 'bf16', groups=3))
    return out


PLANS = [sp for m in MODELS for s in (64, 128, 256) for sp in modes(m, s, s)]
PLANS += modes('UNet', 320, 320) + modes('UNet', 160, 176)
# one switch off at a time, on the training and on the stacked plan (the storage switches only act under bf16)
PLANS += [spec('fuseunet', n, 256, 256, True, 'bf16' if k.startswith('store_') else 'fp32', groups=g, **{k: False})
          for k in SWITCHES for n, g in ((2, 1), (6, 3))]


def make_net(sp, dev=None):
    from aide_amd import models_twomodalinputs, models_singlemodalinput
    torch.manual_seed(0)
    mod = models_twomodalinputs if sp['model'] in TWO_MODAL else models_singlemodalinput
    net = getattr(mod, sp['model'])(2)
    if dev is not None:
        net = net.to(dev)
    net.engine.precision = sp['precision']
    for k, v in sp['config'].items():
        setattr(net.engine.config, k, v)
    net.train(sp['training'])
    return net


def has_backward(sp):
    return sp['training'] and sp['groups'] == 1


def read_plan(sp, dev):
    net = make_net(sp, dev)
    x = torch.empty(sp['n'], 3, sp['h'], sp['w'], device=dev)
    plan = net.engine.plan_for([x] * (2 if sp['model'] in TWO_MODAL else 1), sp['groups'])
    bwd = has_backward(sp)
    if bwd:
        plan._prepare_backward()
    index = {id(st): i for i, st in enumerate(plan.steps)}

    def step(o):
        return None if o is None else index[id(o)]

    def rng(t):
        return None if t is None else [t.c0, t.C]

    steps = []
    for st in plan.steps:
        sg = st.get('src_grad') if bwd else None
        d = dict(kind=st['kind'], lazy_to=step(st.get('lazy_to')), tab_c0=st.get('tab_c0'), head_lazy=bool(st.get('head_lazy')),
                 lazy_prod=step(st.get('lazy_prod')), pool_out=rng(st.get('pool_out')), fwd_fused=bool(st.get('fwd_fused')),
                 src_grad=None if sg is None else [bool(sg['accumulate']), [rng(g) for g in sg['gaps']]],
                 fold_dgrad=bool(bwd and st.get('fold_dgrad')), pool_fuse=rng(st.get('pool_fuse')) if bwd else None,
                 bwd_fused=bool(bwd and st.get('bwd_fused')), head_fuse=step(st.get('head_fuse')) if bwd else None,
                 dgrad_fused=bool(bwd and st.get('dgrad_fused')))
        steps.append([d[k] for k in KEYS])
    roots = [[plan.act[id(t)].dtype == torch.bfloat16, bool(plan.narrow_grad.get(id(t)))] for t in plan.g.roots]
    return dict(spec=sp, lazy_bn=plan.lazy_bn, roots=roots, steps=steps)


def check_not_vacuous(plans):
    """each decision is taken in some step and not taken in another step of its kind; each storage form has a root"""
    col = lambda k, pred: {bool(r[KEYS.index(k)] is not None if k in ('lazy_to', 'head_fuse') else r[KEYS.index(k)])
                           for p in plans for r in p['steps'] if pred(r)}
    conv, pool = (lambda r: r[0] == 'conv'), (lambda r: r[0] == 'pool')
    for k, pred in (('lazy_to', conv), ('head_lazy', conv), ('head_fuse', conv), ('fold_dgrad', conv),
                    ('fwd_fused', pool), ('bwd_fused', pool)):
        assert col(k, pred) == {False, True}, (k, col(k, pred))
    acc = {r[KEYS.index('src_grad')][0] for p in plans for r in p['steps'] if r[KEYS.index('src_grad')] is not None}
    assert acc == {False, True}, acc
    for i, what in enumerate(('activation', 'gradient')):
        assert {r[i] for p in plans for r in p['roots']} == {False, True}, what


DEFAULTS = dict(lazy_to=None, tab_c0=None, head_lazy=False, lazy_prod=None, pool_out=None, fwd_fused=False,
                src_grad=None, fold_dgrad=False, pool_fuse=None, bwd_fused=False, head_fuse=None, dgrad_fused=False)


def pack(plans):
    """full rows (read_plan) -> (kinds per model, packed plans)"""
    kinds, out = {}, []
    for p in plans:
        k = [r[0] for r in p['steps']]
        assert kinds.setdefault(p['spec']['model'], k) == k
        steps = {}
        for i, r in enumerate(p['steps']):
            d = {key: v for key, v in zip(KEYS[1:], r[1:]) if v != DEFAULTS[key] or type(v) is not type(DEFAULTS[key])}
            if d:
                steps[str(i)] = d
        roots = [len(p['roots'])] + [[i for i, r in enumerate(p['roots']) if r[j]] for j in (0, 1)]
        out.append(dict(spec=p['spec'], lazy_bn=p['lazy_bn'], roots=roots, steps=steps))
    return kinds, out


def unpack(fixture):
    """the loaded fixture -> plans with full rows: steps [[value per KEYS entry] per step], roots [[act bf16, grad bf16] per root]"""
    assert tuple(fixture['keys']) == KEYS and fixture['defaults'] == DEFAULTS
    out = []
    for p in fixture['plans']:
        steps = [[kind] + [p['steps'].get(str(i), {}).get(k, DEFAULTS[k]) for k in KEYS[1:]]
                 for i, kind in enumerate(fixture['kinds'][p['spec']['model']])]
        assert all(int(i) < len(steps) and set(d) <= set(DEFAULTS) for i, d in p['steps'].items())
        nroots, act, grad = p['roots']
        out.append(dict(spec=p['spec'], lazy_bn=p['lazy_bn'], roots=[[i in act, i in grad] for i in range(nroots)], steps=steps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit this tree is (stated in the fixture)')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    plans = [read_plan(sp, dev) for sp in PLANS]
    check_not_vacuous(plans)
    kinds, packed = pack(plans)
    with open(args.out, 'w') as f:
        f.write('{"commit": %s,\n "keys": %s,\n "defaults": %s,\n "kinds": {\n%s},\n "plans": [\n' % (
            json.dumps(args.commit), json.dumps(list(KEYS)), json.dumps(DEFAULTS),
            ',\n'.join('  %s: %s' % (json.dumps(m), json.dumps(k)) for m, k in kinds.items())))
        f.write(',\n'.join('  ' + json.dumps(p, separators=(',', ':')) for p in packed))
        f.write('\n ]}\n')
    with open(args.out) as f:
        assert unpack(json.load(f)) == json.loads(json.dumps(plans))      # (the packing is lossless)
    print('%s: %d plans, %d steps, %d bytes' % (args.out, len(plans), sum(len(p['steps']) for p in plans),
                                                os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
