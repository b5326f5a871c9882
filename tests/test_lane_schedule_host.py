"""CPU: engine.lane_schedule -- where the two-lane forward pass launches, forks, joins, records and waits -- against fixture g30
(tools/gen_golden_lane_schedule.py: the stream calls of Plan._forward_impl logged on a GPU, on the commit the fixture names),
against a vector-clock checker of the scheduler's contract, and against hand-written cases.  No library launch, no device.

The contract: of two ops on different streams that touch overlapping channels, at least one of them writing, the
later is ordered behind the earlier; at the end the main stream has seen all of the lane stream's work; and the op at the gate
sees the gate's wait, which is made on the main stream."""
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g30_lane_schedule.json')
LANES = ((False, False), (True, False), (True, True))          # (dual, free)


@pytest.fixture(scope='module')
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def gen():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import gen_golden_lane_schedule as G
    finally:
        sys.path.pop(0)
    return G


def _graph(G, model):
    eng = G.make_net(dict(model=model, training=True, dual_fwd=True, free_lane=True)).engine
    eng._refresh_params()
    return eng.graph


def test_lane_schedule_matches_fixture(fixture, gen):
    """action by action: G.entries() maps every action to its one log entry (none for the gate and for the halves of a pooling
    its producers wrote)"""
    from aide_amd.engine import lane_schedule, gate_step
    assert len(fixture['commit']) == 40 and len(fixture['plans']) == 20
    graphs = {}
    for p in fixture['plans']:
        sp = p['spec']
        ops_ = graphs.setdefault(sp['model'], _graph(gen, sp['model'])).ops
        assert len(ops_) == p['nsteps']
        dual = sp['dual_fwd'] and any(o.get('lane') for o in ops_)           # (Plan: a lane stream only where lane-1 ops are)
        acts = lane_schedule(ops_, dual, dual and sp['free_lane'], gate_step(ops_))
        got = [e for a in acts for e in gen.entries(a, p['fused_split_pools'])]
        assert got == p['log'], sp


def test_fixture_is_not_vacuous(fixture, gen):
    gen.check_not_vacuous(fixture['plans'])
    assert [(p['spec']['dual_fwd'], p['spec']['free_lane']) for p in fixture['plans'][:3]] == list(LANES)


def check(steps, acts, gate_index, dual=True):
    """The vector-clock checker.  A clock is [main-stream launches seen, lane-stream launches seen]; each stream has one.  A launch
    ticks its own stream's entry and keeps the clock as its stamp; fork / join / wait merge a clock into a stream's, record
    snapshots the lane's.  An earlier launch happened before a later one on the other stream iff the later one's stamp has
    reached the earlier one's own entry.  -> number of conflicting pairs checked"""
    clock = [[0, 0], [0, 0]]
    merge = lambda into, other: [max(a, b) for a, b in zip(into, other)]
    snap, done, launched, gate_at, pairs = {}, [], [], None, 0
    from aide_amd.engine import _overlap
    for a in acts:
        kind = a[0]
        if kind == 'fork':
            clock[1] = merge(clock[1], clock[0])
        elif kind == 'join':
            clock[0] = merge(clock[0], clock[1])
        elif kind == 'record':
            snap[a[1]] = list(clock[1])
        elif kind == 'wait':
            clock[0] = merge(clock[0], snap[a[1]])
        elif kind == 'gate':
            clock[0][0] += 1
            gate_at = clock[0][0]
        else:
            i, lane = a[1], a[2]
            st = steps[i]
            src, dst = st['src'], st.get('dst')
            if kind == 'pool_half':
                c = st['lane_split']
                c0, nc = (c, src.C - c) if lane else (0, c)
                src, dst = src.slice(c0, nc), dst.slice(c0, nc)
            else:
                assert kind == 'op'
            clock[lane][lane] += 1
            stamp = list(clock[lane])
            if i == gate_index:
                assert gate_at is not None and stamp[0] >= gate_at, 'step %d does not see the gate' % i
            for lane2, stamp2, src2, dst2 in done:
                conflict = (dst is not None and (_overlap(dst, src2) or (dst2 is not None and _overlap(dst, dst2)))) or \
                    (dst2 is not None and _overlap(dst2, src))
                if lane2 != lane and conflict:
                    pairs += 1
                    assert stamp[lane2] >= stamp2[lane2], 'step %d (lane %d) is not ordered behind an earlier conflicting op' % (i, lane)
            done.append((lane, stamp, src, dst))
            launched.append((kind, i, lane))
    assert clock[0][1] == clock[1][1], 'the main stream has not seen all of the lane stream at the end'
    # every step runs once, in graph order: whole on its own lane, or as its two halves (lane 1 first)
    assert [x[1] for x in launched] == sorted(x[1] for x in launched)
    for i, st in enumerate(steps):
        whole = [('op', i, st.get('lane', 0) if dual else 0)]
        assert [x for x in launched if x[1] == i] in (whole, [('pool_half', i, 1), ('pool_half', i, 0)])
    return pairs


def without_split(steps):
    return [dict(st, lane_split=None) if 'lane_split' in st else st for st in steps]


def random_graph(rng):
    """3 to 9 ops over 8-channel roots: convs on either lane and up-samplings between whole and half slices, whole and split
    poolings (lane_split = 4)"""
    from aide_amd.engine import Graph
    g = Graph()
    roots = [g.tensor('r%d' % k, 8, 0) for k in range(rng.randint(3, 5))]
    part = lambda t: t if rng.random() < 0.4 else t.slice(*rng.choice(((0, 4), (4, 4))))
    for _ in range(rng.randint(3, 9)):
        a, b = rng.sample(roots, 2)
        r = rng.random()
        if r < 0.6:
            g.conv_bn_relu(part(a), part(b), None, None, lane=rng.randint(0, 1))
        elif r < 0.85:
            g.pool(a, b, lane_split=4 if rng.random() < 0.7 else None)
        else:
            s = part(a)
            g.upsample(s, b if s.C == 8 else b.slice(*rng.choice(((0, 4), (4, 4)))))
    return g


def test_contract_on_fuseunet(gen):
    from aide_amd.engine import lane_schedule, gate_step
    ops_ = _graph(gen, 'fuseunet').ops
    for dual, free in LANES:
        pairs = check(ops_, lane_schedule(ops_, dual, free, gate_step(ops_)), gate_step(ops_), dual)
        assert (pairs > 0) == dual


def test_contract_on_random_graphs():
    """one tracker: both settings of `free` hold the contract on every graph, with the gate anywhere or nowhere"""
    from aide_amd.engine import lane_schedule
    rng = random.Random(30)
    pairs = splits = 0
    for _ in range(2500):
        ops_ = random_graph(rng).ops
        convs = [i for i, o in enumerate(ops_) if o['kind'] == 'conv']
        gate = rng.choice(convs) if convs and rng.random() < 0.5 else None
        for free in (False, True):
            acts = lane_schedule(ops_, True, free, gate)
            pairs += check(ops_, acts, gate)
            splits += sum(1 for a in acts if a[0] == 'record')
            assert free or not any(a[0] in ('pool_half', 'record', 'wait') for a in acts)
        assert lane_schedule(ops_, False, False, gate) == [x for i in range(len(ops_))
                                                           for x in ([('gate',)] if i == gate else []) + [('op', i, 0)]]
        assert lane_schedule(ops_, True, False, gate) == lane_schedule(without_split(ops_), True, True, gate)
    assert pairs > 5000 and splits > 500          # (the graphs do conflict across the lanes, and do pool in halves)


def test_free_off_is_free_on_without_lane_split(gen):
    from aide_amd.engine import lane_schedule, gate_step
    ops_ = _graph(gen, 'fuseunet').ops
    assert any(o.get('lane_split') for o in ops_)
    assert lane_schedule(ops_, True, False, gate_step(ops_)) == lane_schedule(without_split(ops_), True, True, gate_step(ops_))
    assert lane_schedule(ops_, True, False, gate_step(ops_)) != lane_schedule(ops_, True, True, gate_step(ops_))


def _case(build):
    from aide_amd.engine import Graph
    g = Graph()
    t = {k: g.tensor(k, 8, 0) for k in 'ABCDEPQRS'}
    build(g, t)
    return g.ops


FORK, JOIN, GATE = ('fork',), ('join',), ('gate',)
lo, hi = (lambda t: t.slice(0, 4)), (lambda t: t.slice(4, 4))
CASES = {
    # lane 1 writes a slice lane 0 read (WAR): the fork orders it behind the read, the trailing join closes the lane
    'lane1_writes_what_lane0_read': (lambda g, t: (g.conv_bn_relu(lo(t['A']), t['B'], None, None),
                                                   g.conv_bn_relu(t['C'], t['A'], None, None, lane=1)), None,
                                     [('op', 0, 0), FORK, ('op', 1, 1), JOIN]),
    # lane 0 writes a slice lane 1 read: a join before the write; nothing of lane 1 is pending at the end
    'lane0_writes_what_lane1_read': (lambda g, t: (g.conv_bn_relu(hi(t['A']), t['B'], None, None, lane=1),
                                                   g.conv_bn_relu(t['C'], t['A'], None, None)), None,
                                     [FORK, ('op', 0, 1), JOIN, ('op', 1, 0)]),
    # two split pools in a row: lane 1 goes from level to level on its own; no wait -- main reads none of lane 1's channels
    'two_split_pools': (lambda g, t: (g.conv_bn_relu(t['A'], hi(t['S']), None, None, lane=1), g.pool(t['S'], t['P'], lane_split=4),
                                      g.pool(t['P'], t['Q'], lane_split=4)), None,
                        [FORK, ('op', 0, 1), ('pool_half', 1, 1), ('record', 1), ('pool_half', 1, 0),
                         ('pool_half', 2, 1), ('record', 2), ('pool_half', 2, 0), JOIN]),
    # ... and main waits for the one event whose channels it reads
    'wait_for_the_pooled_half': (lambda g, t: (g.conv_bn_relu(t['A'], hi(t['S']), None, None, lane=1), g.pool(t['S'], t['P'], lane_split=4),
                                               g.pool(t['P'], t['Q'], lane_split=4), g.conv_bn_relu(t['P'], t['B'], None, None)), None,
                                 [FORK, ('op', 0, 1), ('pool_half', 1, 1), ('record', 1), ('pool_half', 1, 0),
                                  ('pool_half', 2, 1), ('record', 2), ('pool_half', 2, 0), ('wait', 1), ('op', 3, 0), JOIN]),
    # a split pool before any fork runs whole on the main stream: lane 1 has produced nothing
    'split_pool_before_any_fork': (lambda g, t: (g.pool(t['S'], t['P'], lane_split=4),), None, [('op', 0, 0)]),
    # the gate on a lane-1 conv: its lane is forked again behind the wait
    'gate_on_lane1': (lambda g, t: (g.conv_bn_relu(t['A'], t['B'], None, None, lane=1), g.conv_bn_relu(t['B'], t['C'], None, None, lane=1)), 1,
                      [FORK, ('op', 0, 1), GATE, FORK, ('op', 1, 1), JOIN]),
    # the gate on a lane-0 conv: the wait is on its own stream; the next lane-1 op forks again all the same
    'gate_on_lane0': (lambda g, t: (g.conv_bn_relu(t['A'], t['B'], None, None, lane=1), g.conv_bn_relu(t['D'], t['E'], None, None),
                                    g.conv_bn_relu(t['B'], t['C'], None, None, lane=1)), 1,
                      [FORK, ('op', 0, 1), GATE, ('op', 1, 0), FORK, ('op', 2, 1), JOIN]),
    # disjoint slices of one root written by both lanes: nothing between them
    'disjoint_slices_of_one_root': (lambda g, t: (g.conv_bn_relu(t['A'], hi(t['R']), None, None, lane=1),
                                                  g.conv_bn_relu(t['B'], lo(t['R']), None, None)), None,
                                    [FORK, ('op', 0, 1), ('op', 1, 0), JOIN]),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_hand_written_case(name):
    from aide_amd.engine import lane_schedule
    build, gate, want = CASES[name]
    ops_ = _case(build)
    acts = lane_schedule(ops_, True, True, gate)
    assert acts == want
    check(ops_, acts, gate)
    json.dumps(acts)
    assert lane_schedule(ops_, False, True, gate) == [x for i in range(len(ops_)) for x in ([GATE] if i == gate else []) + [('op', i, 0)]]


def test_no_gate_with_at_most_four_convs():
    from aide_amd.engine import lane_schedule, gate_step

    def chain(n):
        return _case(lambda g, t: [g.conv_bn_relu(t['A'], t['B'], None, None, lane=k % 2) for k in range(n)] + [g.pool(t['B'], t['C'])])
    assert gate_step(chain(4)) is None and GATE not in lane_schedule(chain(4), True, True, gate_step(chain(4)))
    five = chain(5)
    assert gate_step(five) == 4 and lane_schedule(five, True, True, 4).count(GATE) == 1
    assert lane_schedule(five, True, True, 4).index(GATE) < lane_schedule(five, True, True, 4).index(('op', 4, 0))
