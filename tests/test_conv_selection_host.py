"""CPU: engine.select_conv against fixture g26 (tools/gen_golden_conv_selection.py: the per-layer kernel-family decisions read
from plans built on a GPU, on the commit the fixture names).  The test walks each model's graph, hands select_conv what
Plan.__init__ hands it, and wants every decision of every conv layer equal -- host-side queries of the library only."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g26_conv_selection.json')


@pytest.fixture(scope='module')
def built():
    from aide_amd.build import build
    return build(verbose=False)


@pytest.fixture(scope='module')
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _select_all(sp):
    """select_conv for every conv of the plan `sp` describes, in graph order -> (rows as dicts, sk_ws of the plan)"""
    from aide_amd.engine import select_conv
    from aide_amd.models_twomodalinputs import fuseunet
    from aide_amd.models_singlemodalinput import UNet
    net = dict(fuseunet=fuseunet, UNet=UNet)[sp['model']](2)
    eng = net.engine
    eng.precision = sp['precision']
    for k, v in sp['config'].items():
        setattr(eng.config, k, v)
    eng._refresh_params()
    cfg, n, size, training, groups = eng.config, sp['n'], sp['size'], sp['training'], sp['groups']
    forward_only = (groups > 1 or not training) and cfg.shared_packs
    rows, stem_only, max_sk = [], True, 0
    for op in eng.graph.ops:
        if op['kind'] == 'conv':
            src, dst = op['src'], op['dst']
            need_dgrad = not src.root.is_input and not forward_only
            d = select_conv(cfg, sp['precision'], training, groups, n, src.C, dst.C, size >> dst.level, size >> dst.level,
                            need_dgrad, stem_only)
            max_sk = max(max_sk, d['sk_f'], d['sk_d'])
            rows.append(d)
        stem_only = stem_only and op['kind'] == 'conv' and op['src'].root.is_input
    return rows, max(max_sk // 4, 1)


def test_select_conv_matches_fixture(built, fixture):
    keys = fixture['keys']
    assert len(fixture['commit']) == 40 and len(fixture['plans']) >= 23
    for p in fixture['plans']:
        rows, sk_ws = _select_all(p['spec'])
        assert len(rows) == len(p['convs']), p['spec']
        for i, (got, want) in enumerate(zip(rows, p['convs'])):
            for k, v in zip(keys, want):
                assert got[k] == v and type(got[k]) is type(v), '%s conv %d %s: %r, fixture %r' % (p['spec'], i, k, got[k], v)
        assert sk_ws == p['sk_ws'], p['spec']


def test_fixture_is_not_vacuous(fixture):
    BF16 = 16                        # aide_amd.ops.BF16 (a constant: no library needed here)
    col = {k: [r[i] for p in fixture['plans'] for r in p['convs']] for i, k in enumerate(fixture['keys'])}
    for k in ('wino_f', 'wino_d', 'wino_w'):
        assert set(col[k]) == {0, 2, 4, BF16}, (k, sorted(set(col[k])))
    assert 256 in col['wg_target']
    assert max(col['stats_parts']) > 0
    folded = {m for m, f in zip(col['wino_f'], col['fold']) if f}
    assert 0 in folded and 4 in folded
