"""The launch sequences of four fuseunet plans against fixture g27 (tools/gen_golden_launch_trace.py, recorded on the commit the
fixture names): entry-point names, their order and every scalar argument of the forward and backward launch tapes, and the
(n, total_blocks) of every kernel family's filter-pack tables.  Equality, no tolerance: host-side refactors of the engine must
not move a launch."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g27_launch_trace.json')


@pytest.fixture(scope='module')
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['train_fp32', 'train_bf16', 'eval_fp32', 'stacked_fp32'])
def test_launch_trace_matches_fixture(dev, fixture, name):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import gen_golden_launch_trace as G
    finally:
        sys.path.pop(0)
    want = fixture['plans'][name]
    got = json.loads(json.dumps(G.trace(*(G.PLANS[name] + (dev,)))))       # (tuples -> lists, as the fixture went through JSON)
    assert sorted(got) == sorted(want)
    assert got['packs'] == want['packs']
    for k in ('forward', 'backward'):
        if k in want:
            assert len(want[k]) > 50
            for i, (g, w) in enumerate(zip(got[k], want[k])):
                assert g == w, '%s %s, launch %d: %r, fixture %r' % (name, k, i, g, w)
            assert len(got[k]) == len(want[k])
