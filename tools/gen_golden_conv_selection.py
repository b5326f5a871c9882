"""Writes tests/golden/g26_conv_selection.json: the per-layer kernel-family decisions of the engine's plans.

    python tools/gen_golden_conv_selection.py --commit $(git rev-parse HEAD)

Needs a GPU (plans own device buffers).  For every plan of PLANS it reads, for every conv step, the decisions KEYS names from
the plan's step dicts -- only keys every tree since 82d7905 stores, so the same script runs on an older commit: the committed
fixture states the commit it was generated on, and tests/test_conv_selection_host.py holds engine.select_conv to it on the
host.  `z_bf16` is the storage type of the step's z, `sk_f` / `sk_d` the split-K workspace bytes of the two directions (what
Plan.__init__ takes the maximum of), `sk_ws` the plan's resulting workspace in floats."""
import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aide_amd._lib import lib  # noqa: E402
from aide_amd.engine import BF16  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'g26_conv_selection.json')
KEYS = ('wino_f', 'wino_d', 'wino_w', 'plan_f', 'plan_d', 'wg_target', 'wg_bytes', 'stats_parts', 'fold', 'dz_bf16', 'z_bf16',
        'sk_f', 'sk_d')


def spec(model, n, size, training, precision, groups=1, **config):
    return dict(model=model, n=n, size=size, training=training, precision=precision, groups=groups, config=config)


PLANS = [spec('fuseunet', 2, s, tr, p) for tr in (True, False) for p in ('fp32', 'bf16') for s in (64, 128, 256)]
PLANS += [spec('fuseunet', 6, s, True, p, groups=3) for p in ('fp32', 'bf16') for s in (64, 128, 256)]
PLANS += [spec('UNet', 2, 320, True, 'fp32')]                        # the 20x20 bottleneck canvas
PLANS += [spec('fuseunet', 2, 128, True, 'fp32', **{k: False})
          for k in ('use_winograd', 'use_winograd4', 'use_winograd_dgrad', 'w4_half_tile')]


def make_net(sp, dev=None):
    from aide_amd.models_twomodalinputs import fuseunet
    from aide_amd.models_singlemodalinput import UNet
    torch.manual_seed(0)
    net = dict(fuseunet=fuseunet, UNet=UNet)[sp['model']](2)
    if dev is not None:
        net = net.to(dev)
    net.engine.precision = sp['precision']
    for k, v in sp['config'].items():
        setattr(net.engine.config, k, v)
    net.train(sp['training'])
    return net


def rows(sp, dev):
    net = make_net(sp, dev)
    n, s = sp['n'], sp['size']
    x = torch.empty(n, 3, s, s, device=dev)
    plan = net.engine.plan_for([x] * (2 if sp['model'] == 'fuseunet' else 1), sp['groups'])
    out = []
    for st in plan.steps:
        if st['kind'] != 'conv':
            continue
        hh, ww = s >> st['dst'].level, s >> st['dst'].level
        dgrad = st['wd'] is not None or st['ud'] is not None
        d = dict(wino_f=st['wino_f'], wino_d=st['wino_d'], wino_w=st['wino_w'], plan_f=st['plan_f'], plan_d=st['plan_d'],
                 wg_target=st.get('wg_target', 0), wg_bytes=st['wg_bytes'], stats_parts=st.get('stats_parts', 0),
                 fold=bool(st['fold']), dz_bf16=bool(st['dz_bf16']),
                 z_bf16=st['z'] is not None and st['z'].dtype == torch.bfloat16,
                 sk_f=lib.aide_conv3x3_ws_bytes(n, hh, ww, st['dst'].C, st['plan_f'] >> 8),
                 sk_d=lib.aide_conv3x3_ws_bytes(n, hh, ww, st['src'].C, st['plan_d'] >> 8) if dgrad else 0)
        out.append([d[k] for k in KEYS])
    return out, plan.sk_ws.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit this tree is (stated in the fixture)')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    plans = []
    for sp in PLANS:
        convs, sk_ws = rows(sp, dev)
        plans.append(dict(spec=sp, sk_ws=sk_ws, convs=convs))
    col = {k: [r[i] for p in plans for r in p['convs']] for i, k in enumerate(KEYS)}
    for k in ('wino_f', 'wino_d', 'wino_w'):                          # the fixture is not vacuous
        assert set(col[k]) == {0, 2, 4, BF16}, (k, sorted(set(col[k])))
    assert 256 in col['wg_target'] and max(col['stats_parts']) > 0
    assert {m for m, f in zip(col['wino_f'], col['fold']) if f} >= {0, 4}
    with open(args.out, 'w') as f:
        f.write('{"commit": %s,\n "keys": %s,\n "plans": [\n' % (json.dumps(args.commit), json.dumps(list(KEYS))))
        f.write(',\n'.join('  {"spec": %s, "sk_ws": %d, "convs": [\n%s]}' % (
            json.dumps(p['spec']), p['sk_ws'], ',\n'.join('   ' + json.dumps(r) for r in p['convs'])) for p in plans))
        f.write('\n ]}\n')
    print('%s: %d plans, %d conv layers' % (args.out, len(plans), len(col['wino_f'])))


if __name__ == '__main__':
    main()
