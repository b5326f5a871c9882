"""The launch sequences of four fuseunet plans at 128x128 against fixture g27, and of the training and the stacked plan at 256x256
-- where the conv-epilogue statistics and with them the lazy BatchNorm paths fire -- against g29 (tools/gen_golden_launch_trace.py,
recorded on the commit each fixture names): entry-point names, their order and every scalar argument of the forward and backward
launch tapes, and the (n, total_blocks) of every kernel family's filter-pack tables.  Equality, no tolerance: host-side
refactors of the engine must not move a launch.

The stream every backward launch, hand-over, flush and join goes to, and where the per-step callbacks run, against g31
(tools/gen_golden_backward_schedule.py): the 64x64 plans regenerated, flush entries included."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g27_launch_trace.json')


FIXTURE_256 = os.path.join(ROOT, 'tests', 'golden', 'g29_launch_trace_256.json')


@pytest.fixture(scope='module')
def fixture():
    plans = {}
    for path in (FIXTURE, FIXTURE_256):
        with open(path) as f:
            plans.update(json.load(f)['plans'])
    return dict(plans=plans)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['train_fp32', 'train_bf16', 'eval_fp32', 'stacked_fp32',
                                  'train_fp32_256', 'stacked_fp32_256'])
def test_launch_trace_matches_fixture(dev, fixture, name):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import gen_golden_launch_trace as G
    finally:
        sys.path.pop(0)
    want = fixture['plans'][name]
    args = G.PLANS[name] if name in G.PLANS else G.PLANS_256[name]
    got = json.loads(json.dumps(G.trace(*(args + (dev,)))))       # (tuples -> lists, as the fixture went through JSON)
    assert sorted(got) == sorted(want)
    assert got['packs'] == want['packs']
    for k in ('forward', 'backward'):
        if k in want:
            assert len(want[k]) > 50
            for i, (g, w) in enumerate(zip(got[k], want[k])):
                assert g == w, '%s %s, launch %d: %r, fixture %r' % (name, k, i, g, w)
            assert len(got[k]) == len(want[k])


@pytest.mark.gpu
def test_backward_streams_match_fixture(dev):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import gen_golden_backward_schedule as G
    finally:
        sys.path.pop(0)
    with open(G.OUT) as f:
        want = G.unpack(json.load(f))
    small = [p for p in want if p['spec']['h'] == 64]
    assert len(small) == 8 and [p['spec'] for p in want] == G.PLANS
    for p in small:
        got = json.loads(json.dumps(G.read_plan(p['spec'], dev)))
        assert got['nsteps'] == p['nsteps'] and len(got['log']) == len(p['log']) > 100, p['spec']
        for i, (g, w) in enumerate(zip(got['log'], p['log'])):
            assert g == w, '%s, entry %d: %r, fixture %r' % (p['spec'], i, g, w)
