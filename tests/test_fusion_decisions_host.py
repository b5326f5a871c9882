"""CPU: engine.select_fusions against fixture g28 (tools/gen_golden_fusion_decisions.py: the fusion, storage and backward-write
decisions read from plans built on a GPU, on the commit the fixture names).  The test walks each model's graph, hands
select_conv and select_fusions what Plan.__init__ hands them, and wants every recorded value of every step and root equal,
types included -- host-side queries of the library only.  (The fixture is stored packed: the generator's unpack() gives
the full rows back.)"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g28_fusion_decisions.json')


@pytest.fixture(scope='module')
def built():
    from aide_amd.build import build
    return build(verbose=False)


@pytest.fixture(scope='module')
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def gen():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import gen_golden_fusion_decisions as G
    finally:
        sys.path.pop(0)
    return G


def _decide(G, sp):
    """select_conv per conv and select_fusions once, as Plan.__init__ calls them -> (graph, select_fusions' result)"""
    from aide_amd.engine import select_conv, select_fusions
    eng = G.make_net(sp).engine
    eng._refresh_params()
    cfg, n, h, w, training, groups = eng.config, sp['n'], sp['h'], sp['w'], sp['training'], sp['groups']
    forward_only = (groups > 1 or not training) and cfg.shared_packs
    convs, stem_only = {}, True
    for i, op in enumerate(eng.graph.ops):
        if op['kind'] == 'conv':
            src, dst = op['src'], op['dst']
            need_dgrad = not src.root.is_input and not forward_only
            convs[i] = select_conv(cfg, sp['precision'], training, groups, n, src.C, dst.C, h >> dst.level, w >> dst.level,
                                   need_dgrad, stem_only)
        stem_only = stem_only and op['kind'] == 'conv' and op['src'].root.is_input
    return eng.graph, select_fusions(eng.graph, convs, cfg, sp['precision'], training, groups, n, h, w)


def test_select_fusions_matches_fixture(built, fixture, gen):
    keys = fixture['keys']
    assert len(fixture['commit']) == 40 and len(fixture['plans']) >= 89
    for p in gen.unpack(fixture):
        sp = p['spec']
        graph, fus = _decide(gen, sp)
        assert len(fus['steps']) == len(p['steps']) == len(graph.ops), sp
        for i, (op, d, want) in enumerate(zip(graph.ops, fus['steps'], p['steps'])):
            got = dict(d, kind=op['kind'])
            for k in ('pool_out', 'pool_fuse'):          # [root, c0, C]; the fixture records the slice within the root
                if got[k] is not None:       # (the root: test_fused_slices_lie_in_the_pooled_root)
                    got[k] = got[k][1:]
            for k, v in zip(keys, want):
                assert got[k] == v and type(got[k]) is type(v), '%s step %d %s: %r, fixture %r' % (sp, i, k, got[k], v)
        roots = [[a, g] for a, g in zip(fus['act_bf16'], fus['grad_bf16'])]
        assert roots == p['roots'] and all(type(x) is bool for r in roots for x in r), sp
        assert sum(1 for d in fus['steps'] if d['lazy_to'] is not None) == p['lazy_bn'], sp


def test_fused_slices_lie_in_the_pooled_root(built, fixture, gen):
    """the root select_fusions names for pool_out / pool_fuse (the fixture holds only the slice) is the pooling's destination"""
    for p in gen.unpack(fixture)[:12]:
        graph, fus = _decide(gen, p['spec'])
        pooled = {id(op['src'].root): graph.roots.index(op['dst'].root) for op in graph.ops if op['kind'] == 'pool'}
        for op, d in zip(graph.ops, fus['steps']):
            for k in ('pool_out', 'pool_fuse'):
                if d[k] is not None:
                    assert d[k][0] == pooled[id(op['dst'].root)], (p['spec'], k)


def test_fixture_is_not_vacuous(fixture, gen):
    assert tuple(fixture['keys']) == gen.KEYS
    gen.check_not_vacuous(gen.unpack(fixture))
