"""CPU: engine.backward_schedule -- what the backward pass launches on which stream, and every fork, hand-over, flush point and
join -- against fixture g31 (tools/gen_golden_backward_schedule.py: the recorded backward tapes of plans run on a GPU, on the
commit the fixture names, reduced to entry point, stream roles and callbacks), against a vector-clock checker of the schedule's
contract, and against hand-written cases.  Host-side queries of the library only, no device.

The contract: a weight gradient on another stream than the BatchNorm backward of its step is ordered behind it; a
weight gradient that records its slab reduce into the queue is followed by a flush point on a stream that has seen it; a step's
callback comes after every launch of the step and, where the reduces run batched, after such a flush point; every step runs
once, in reversed graph order; only the tail weight gradient is unqueued on the main stream beside a weight-gradient stream;
and at the end the main stream has seen all of the weight-gradient stream's work."""
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g31_backward_schedule.json')
MODELS = (('fuseunet', False), ('fuseunetsa', False), ('fuseunetsaseparate', False), ('UNet', False), ('UNetsa', False),
          ('fuseunet', True), ('UNet', True))                   # (model, learned_bilinear)
LAUNCHES = ('fill', 'bn', 'wgrad', 'dgrad', 'head', 'op')


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
        import gen_golden_backward_schedule as G
    finally:
        sys.path.pop(0)
    return G


def _steps(G, sp):
    """select_conv per conv and select_fusions once, as Plan.__init__ calls them -> (step dicts with the keys backward_schedule
    reads, src_grad in the form Plan.__init__ gives it; the engine's config)"""
    from aide_amd.engine import select_conv, select_fusions
    eng = G.make_net(sp).engine
    eng._refresh_params()
    cfg, n, h, w = eng.config, sp['n'], sp['h'], sp['w']
    convs, stem_only = {}, True
    for i, op in enumerate(eng.graph.ops):
        if op['kind'] == 'conv':
            src, dst = op['src'], op['dst']
            convs[i] = select_conv(cfg, sp['precision'], True, 1, n, src.C, dst.C, h >> dst.level, w >> dst.level,
                                   not src.root.is_input, stem_only)
        stem_only = stem_only and op['kind'] == 'conv' and op['src'].root.is_input
    fus = select_fusions(eng.graph, convs, cfg, sp['precision'], True, 1, n, h, w)
    steps = []
    for i, (op, d) in enumerate(zip(eng.graph.ops, fus['steps'])):
        sg = d['src_grad']
        steps.append(dict(op, **dict(d, src_grad=sg and dict(accumulate=sg[0], gaps=sg[1]), plan_d=convs.get(i, {}).get('plan_d'))))
    return steps, cfg


def test_backward_schedule_matches_fixture(built, fixture, gen):
    """action by action through G.entries().  The flush entries leave both sides: where they fall depends on queue.pending(), a
    host-state query of the library (fixtures g27 / g29 hold their positions on a GPU); with them the positions of the callbacks
    that wait for a flush -- their order stays.  Everything else, stream roles included, by equality and in place."""
    from aide_amd.engine import backward_schedule
    assert len(fixture['commit']) == 40 and len(fixture['plans']) == len(gen.PLANS) == 9
    for p, sp in zip(gen.unpack(fixture), gen.PLANS):
        assert p['spec'] == sp
        steps, cfg = _steps(gen, sp)
        assert len(steps) == p['nsteps']
        side, tail_main, on_kernel, batched = gen.booleans(sp, cfg)
        acts = backward_schedule(steps, side, tail_main, on_kernel, batched)
        got = [e for a in acts for e in gen.entries(a, steps) if e[0] != gen.FLUSH]
        want = [e for e in gen.launches(p['log']) if e[0] != gen.FLUSH]
        if batched:
            split = lambda log: ([e for e in log if e[0] != 'after'], [e for e in log if e[0] == 'after'])
            assert split(got) == split(want), sp
        else:
            assert got == want, sp
        assert len(got) > 100 and (side or not any('side' in e for e in want))


def test_fixture_is_not_vacuous(fixture, gen):
    gen.check_not_vacuous(gen.unpack(fixture))


def check(steps, acts, side, batched):
    """The vector-clock checker.  A clock is [main-stream launches seen, weight-gradient-stream launches seen]; each stream has
    one.  A launch ticks its own stream's entry and keeps the clock as its stamp; fork / join / wait / order merge a clock into
    a stream's (a `done` event is the stamp of the BatchNorm backward it rides on; `order` records where it stands).  An
    earlier launch happened before a later one on the other stream iff the later one's stamp has reached the earlier one's own
    entry.  -> number of cross-stream pairs checked"""
    clock = [[0, 0], [0, 0]]
    merge = lambda into, other: [max(a, b) for a, b in zip(into, other)]
    pairs, bn, unflushed, order, ended, seen = 0, {}, [], [], set(), set()
    launched = {}                        # step -> [(stream, stamp)] of its launches
    due = []                             # steps whose callback waits for a flush point that follows their weight gradient
    for a in acts:
        kind, i = a[0], a[1] if len(a) > 1 else None
        assert i is None or kind == 'flush' or i not in ended, 'an action of step %d behind its end' % i
        if kind == 'fork':
            assert side
            clock[1] = merge(clock[1], clock[0])
        elif kind == 'join':
            assert side and a is acts[-1]
            clock[0] = merge(clock[0], clock[1])
        elif kind == 'begin':
            assert i not in seen and not launched.get(i)
            seen.add(i)
            order.append(i)
        elif kind == 'wait':
            assert side and bn[i][1], 'step %d: a wait for an event no launch carries' % i
            clock[1] = merge(clock[1], bn[i][0])
        elif kind == 'order':
            assert side and not bn[i][1]
            clock[1] = merge(clock[1], clock[0])
        elif kind == 'flush':
            s = a[2]
            assert batched and s == int(side) and a[3] == (i == 0)
            for st_i, (ws, stamp) in unflushed:          # (a flush point: the flush, if it happens here, sees every queued reduce)
                pairs += ws != s
                assert clock[s][ws] >= stamp[ws], 'the flush point after step %d has not seen the weight gradient of step %d' % (i, st_i)
            if a[3]:                     # the last one flushes whatever is pending
                unflushed, due = [], []
        elif kind == 'end':
            ended.add(i)
            if batched:
                due.append(i)
        else:
            assert kind in LAUNCHES and i in seen
            s = a[2] if kind in ('wgrad', 'head') else 0
            assert s == 0 or side
            clock[s][s] += 1
            stamp = list(clock[s])
            launched.setdefault(i, []).append((s, stamp))
            if kind == 'bn':
                assert a[4] in (False, True) and (a[3] > 0) == (a[2] == 'slabs')
                bn[i] = (stamp, a[4])
            elif kind == 'wgrad':
                if s != 0:               # behind the BatchNorm backward of its own step, which ran on the main stream
                    pairs += 1
                    assert stamp[0] >= bn[i][0][0], 'the weight gradient of step %d is not ordered behind its BatchNorm backward' % i
                if a[3]:
                    assert batched and steps[i]['kind'] == 'conv' and not (side and s == 0)
                    unflushed.append((i, (s, stamp)))
                elif side and s == 0:    # the tail, and only it: the last launch of the pass, a step without a data gradient
                    assert i == 0 and steps[0].get('src_grad') is None and a is [x for x in acts if x[0] in LAUNCHES][-1]
                else:                    # (ConvTranspose: its kernel reduces its own slabs)
                    assert not batched or steps[i]['kind'] == 'convT'
    assert not unflushed and not due, 'a queued weight gradient or a callback without a last flush point'
    assert clock[0][1] == clock[1][1], 'the main stream has not seen all of the weight-gradient stream at the end'
    assert order == list(reversed(range(len(steps)))) and ended == set(order)
    if not side:
        assert not any(a[0] in ('fork', 'join', 'wait', 'order') for a in acts) and all(s == 0 for v in launched.values() for s, _ in v)
    return pairs


def _flush_follows(acts):
    """with `batched`: behind every queued weight gradient, and behind the end of every step, comes a flush point"""
    pos = [k for k, a in enumerate(acts) if a[0] == 'flush']
    for k, a in enumerate(acts):
        if (a[0] == 'wgrad' and a[3]) or a[0] == 'end':
            assert pos and pos[-1] > k and acts[pos[-1]][3]


def test_contract_on_every_model_and_setting(built, gen):
    from aide_amd.engine import backward_schedule
    for model, learned in MODELS:
        for size, precision in ((64, 'fp32'), (256, 'fp32'), (64, 'bf16')):
            steps, _ = _steps(gen, gen.spec(model, size=size, precision=precision, learned=learned))
            for side, tail_main, on_kernel, batched in itertools.product((False, True), repeat=4):
                acts = backward_schedule(steps, side, tail_main, on_kernel, batched)
                json.dumps(acts)
                pairs = check(steps, acts, side, batched)
                assert (pairs > 0) == side, (model, learned, size, precision, side, tail_main, on_kernel, batched)
                if batched:
                    _flush_follows(acts)
                else:
                    assert not any(a[0] == 'flush' or (a[0] == 'wgrad' and a[3]) for a in acts)
                away = [a[1] for a in acts if a[0] == 'wgrad' and a[2] == 1]       # steps that hand their dz over
                stems = steps[0]['kind'] == 'conv' and steps[0].get('src_grad') is None
                assert len(away) == (sum(1 for a in acts if a[0] == 'wgrad') - (tail_main and stems) if side else 0)
                assert [a for a in acts if a[0] in ('wait', 'order')] == [('wait' if on_kernel else 'order', i) for i in away]
                assert all(a[4] == (on_kernel and a[1] in away) for a in acts if a[0] == 'bn')


def _case(build):
    from aide_amd.engine import Graph, NO_FUSION
    g = Graph()
    t = {k: g.tensor(k, 8, 0) for k in 'ABCD'}
    t['X'] = g.input('X', 3)
    build(g, t)
    return [dict(op, **NO_FUSION) for op in g.ops]


def test_slabs_feed_the_batchnorm_backward_of_the_conv_before():
    """two convs in a row, fold_dgrad on the second: the first one's BatchNorm backward reads slabs with the second's split count,
    and nothing else reads slabs"""
    from aide_amd.engine import backward_schedule
    steps = _case(lambda g, t: (g.conv_bn_relu(t['X'], t['A'], None, None), g.conv_bn_relu(t['A'], t['B'], None, None),
                                g.conv_bn_relu(t['B'], t['C'], None, None)))
    for i in (1, 2):
        steps[i].update(src_grad=dict(accumulate=False, gaps=[]), plan_d=(2 + i) << 8)
    steps[2]['fold_dgrad'] = True
    for side, tail_main, on_kernel, batched in itertools.product((False, True), repeat=4):
        acts = backward_schedule(steps, side, tail_main, on_kernel, batched)
        check(steps, acts, side, batched)
        assert [a[1:4] for a in acts if a[0] == 'bn'] == [(2, 'grad', 0), (1, 'slabs', 4), (0, 'grad', 0)]
        assert [a[1:] for a in acts if a[0] == 'dgrad'] == [(2, True), (1, False)]
    assert backward_schedule(steps, True, True, True, True) == [
        ('fork',),
        ('begin', 2), ('bn', 2, 'grad', 0, True), ('wait', 2), ('wgrad', 2, 1, True), ('dgrad', 2, True), ('end', 2), ('flush', 2, 1, False),
        ('begin', 1), ('bn', 1, 'slabs', 4, True), ('wait', 1), ('wgrad', 1, 1, True), ('dgrad', 1, False), ('end', 1), ('flush', 1, 1, False),
        ('begin', 0), ('bn', 0, 'grad', 0, False), ('wgrad', 0, 0, False), ('end', 0), ('flush', 0, 1, True),
        ('join',)]
    assert backward_schedule(steps, True, False, False, False) == [
        ('fork',),
        ('begin', 2), ('bn', 2, 'grad', 0, False), ('order', 2), ('wgrad', 2, 1, False), ('dgrad', 2, True), ('end', 2),
        ('begin', 1), ('bn', 1, 'slabs', 4, False), ('order', 1), ('wgrad', 1, 1, False), ('dgrad', 1, False), ('end', 1),
        ('begin', 0), ('bn', 0, 'grad', 0, False), ('order', 0), ('wgrad', 0, 1, False), ('end', 0),
        ('join',)]


def test_head_over_a_head_fuse_layer_launches_no_data_gradient():
    from aide_amd.engine import backward_schedule
    steps = _case(lambda g, t: (g.conv_bn_relu(t['X'], t['A'], None, None), g.conv_bn_relu(t['A'], t['B'], None, None),
                                g.head(t['B'], None)))
    steps[1].update(src_grad=dict(accumulate=False, gaps=[]), plan_d=1 << 8, head_fuse=2)
    steps[2].update(src_grad=dict(accumulate=False, gaps=[]), dgrad_fused=True)
    for side in (False, True):
        for lazy in (None, 1):
            steps[2]['lazy_prod'] = lazy
            acts = backward_schedule(steps, side, True, True, True)
            check(steps, acts, side, True)
            assert [a for a in acts if a[0] == 'head'] == [('head', 2, int(side), 'wgrad')]
            assert [a[1:3] for a in acts if a[0] == 'bn'] == [(1, 'head'), (0, 'grad')]
    # ... and without the fusion: split across the streams, split in place where the activation is recomputed, else one launch
    steps[1]['head_fuse'], steps[2]['dgrad_fused'] = None, False
    heads = lambda side, lazy: [a[2:] for a in backward_schedule([dict(s, lazy_prod=lazy) if s['kind'] == 'head' else s for s in steps],
                                                                 side, True, True, True) if a[0] == 'head']
    assert heads(True, None) == heads(True, 1) == [(1, 'wgrad'), (0, 'dgrad')]
    assert heads(False, 1) == [(0, 'wgrad'), (0, 'dgrad')]
    assert heads(False, None) == [(0, 'both')]
