"""Kernel-level net under the 3x3 weight gradient (-m gpu): every family that writes per-split slabs, the slab reduce in its
immediate, scalar and queued forms, and the batched launch of aide_wgrad_queue_flush.  Cases, float64 reference and guarded
buffers: tests/wgrad_cases.py (made binding on the host by tests/test_wgrad_cases_host.py).

Layout of every call: dz and a are channel slices from the middle of a [N, C + 2 * PAD, H, W] buffer whose neighbouring planes
hold +-1e30 (finite: a load masked by selection or by a zero multiplier stays correct, a leak shows at once); N == 1 runs dense
(ops.planes() replaces the batch stride there).  ws and dw are views into NaN-filled allocations with 4096 guard words on both
sides, ws sized by the family's own *_ws_bytes query: an element a kernel never writes stays NaN, a write past either end
breaks a guard.

Largest error of each family over its cases, max |dw - ref| / max |ref| against the float64 reference, measured on an MI355X
(tolerances: WC.TOL, the project's own, set against fp32 aten):
    direct     2.6e-07  (1x520>130@8x16)      of 2e-5        stem       2.1e-07  (1x2>20@8x128)      of 2e-5
    wino2      2.0e-07  (2x256>256@6x48)      of 2e-5        wino4      4.8e-06  (2x32>160@12x16-t3) of 1e-4
    bf16       2.0e-07  (1x40>32@8x32)        of 3e-5        stem_bf16  1.7e-07  (2x3>32@64x64)      of 3e-5
    scalar reduce (misaligned dw or ws): at most 2.3e-07, F(4x4) 1.9e-06
Queued and immediate results are compared bit for bit: both run wgrad_reduce_body4 with the same group count, and the reduce
of a single slab is a copy in either kernel."""
import pytest
import torch

import wgrad_cases as WC

pytestmark = pytest.mark.gpu

PAD = 2                        # channel planes on either side of a slice
IDS = [WC.case_id(c) for c in WC.CASES]


def _place(t, bf16, dev):
    """the CPU tensor on the device: dense for N == 1, else the middle channels of a wider buffer with +-1e30 around them"""
    dtype = torch.bfloat16 if bf16 else torch.float32
    n, ch, h, w = t.shape
    if n == 1:
        return t.to(device=dev, dtype=dtype).contiguous()
    big = torch.empty(n, ch + 2 * PAD, h, w, dtype=dtype, device=dev)
    big[:, :PAD] = 1e30
    big[:, PAD + ch:] = -1e30
    big[:, PAD:PAD + ch] = t.to(device=dev, dtype=dtype)
    return big[:, PAD:PAD + ch]


def _device_operands(c, dev):
    """-> (dz, a) as the case stores them (bf16 storage is exact: WC.operands already rounded those values)"""
    x, dz = WC.operands(c)
    dz_b, a_b = WC.stored_bf16(c)
    return _place(dz, dz_b, dev), _place(x, a_b, dev)


def _ws_words(c):
    from aide_amd._lib import lib
    L = lib.load()             # raw entry points: host-side size queries
    dims = (c.n, c.co, c.ci, c.h, c.w)
    if c.family in ('direct', 'stem'):
        b = L.aide_conv3x3_wgrad_ws_bytes(*dims)
    elif c.family == 'wino2':
        b = L.aide_conv3x3_wgrad_wino_ws_bytes(*dims)
    elif c.family == 'wino4':
        b = L.aide_conv3x3_wgrad_wino4_ws_bytes_t(*(dims + (c.target_wgs,)))
    else:
        b = L.aide_conv3x3_wgrad_bf16_ws_bytes(*(dims + (c.co_blocks,)))
    assert b > 0 and b % 4 == 0
    return b // 4


def _launch(c, dz, a, dw, ws, queue=None):
    from aide_amd import ops
    dw4 = dw.view(c.co, c.ci, 3, 3)
    if c.family in ('direct', 'stem'):
        ops.conv3x3_wgrad(dz, a, dw4, ws=ws, queue=queue)
    elif c.family == 'wino2':
        ops.conv3x3_wgrad_wino(dz, a, dw4, ws=ws, queue=queue)
    elif c.family == 'wino4':
        ops.conv3x3_wgrad_wino4(dz, a, dw4, ws=ws, target_wgs=c.target_wgs, queue=queue)
    else:
        ops.conv3x3_wgrad_bf16(dz, a, dw4, ws=ws, queue=queue, co_blocks=c.co_blocks)


class Call(object):
    """one weight-gradient call with its own guarded ws and dw"""

    def __init__(self, c, dev, dw_lead=WC.LEAD, ws_lead=WC.LEAD, operands=None):
        self.c, self.dw_lead, self.ws_lead = c, dw_lead, ws_lead
        self.dz, self.a = operands if operands is not None else _device_operands(c, dev)
        self.nws, self.ndw = _ws_words(c), c.co * c.ci * 9
        self.ws_buf, self.ws = WC.guarded(self.nws, ws_lead, dev)
        self.dw_buf, self.dw = WC.guarded(self.ndw, dw_lead, dev)

    def run(self, queue=None):
        _launch(self.c, self.dz, self.a, self.dw, self.ws, queue)
        return self

    def guards_intact(self):
        """all four guard regions: before and behind ws, before and behind dw"""
        return WC.guards_intact(self.ws_buf, self.ws_lead, self.nws) and WC.guards_intact(self.dw_buf, self.dw_lead, self.ndw)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_NOW = {}


def _now(c, dev):
    """dw of the immediate path (queue=None), computed once per case and left unchanged"""
    if c not in _NOW:
        call = Call(c, dev).run()
        torch.cuda.synchronize()
        assert call.guards_intact(), WC.case_id(c)
        _NOW[c] = call.dw.clone()
    return _NOW[c]


def _flush(q):
    from aide_amd import ops
    q.flush(ops.stream_ptr())
    torch.cuda.synchronize()


def _parity(c, dw, what):
    got = dw.detach().cpu().view(c.co, c.ci, 3, 3)
    assert not bool(torch.isnan(got).any()), '%s %s: NaN in dw (a slab element nobody wrote)' % (what, WC.case_id(c))
    err = WC.rel_err(got, WC.reference(c))
    print('%s %-44s err %.3e (tolerance %.0e)' % (what, WC.case_id(c), err, WC.TOL[c.family]))
    assert err <= WC.TOL[c.family], '%s %s: max abs err %.3e of the reference scale > %.0e' % (
        what, WC.case_id(c), err, WC.TOL[c.family])


@pytest.mark.parametrize('c', WC.CASES, ids=IDS)
def test_parity_guards_and_strides(dev, c):
    call = Call(c, dev).run()
    torch.cuda.synchronize()
    _parity(c, call.dw, 'parity')
    assert call.guards_intact(), 'a write outside ws or dw'
    assert not bool(torch.isnan(call.ws).any()), 'the workspace of *_ws_bytes holds words no split wrote'
    again = Call(c, dev, operands=(call.dz, call.a)).run()          # a fresh NaN-filled workspace
    torch.cuda.synchronize()
    assert _bits_equal(again.dw, call.dw) and again.guards_intact()


@pytest.mark.parametrize('which', ('dw', 'ws'))
@pytest.mark.parametrize('c', [c for c in WC.CASES if c.misaligned], ids=[WC.case_id(c) for c in WC.CASES if c.misaligned])
def test_misaligned_dw_takes_the_scalar_reduce(dev, c, which):
    """dw four bytes off a 16-byte boundary (and, the same condition of aide_wgrad_reduce_launch, the workspace)"""
    from aide_amd import ops
    q = ops.new_wgrad_queue()
    call = Call(c, dev, dw_lead=WC.LEAD_MISALIGNED if which == 'dw' else WC.LEAD,
                ws_lead=WC.LEAD_MISALIGNED if which == 'ws' else WC.LEAD)
    assert call.dw.data_ptr() % 16 == (4 if which == 'dw' else 0) and call.ws.data_ptr() % 16 == (4 if which == 'ws' else 0)
    call.run(queue=q)
    assert q.pending() == 0                     # not queued: the reduce was launched at once
    torch.cuda.synchronize()
    _parity(c, call.dw, 'misaligned ' + which)
    assert call.guards_intact()


@pytest.mark.parametrize('c', WC.CASES, ids=IDS)
def test_queued_equals_immediate(dev, c):
    from aide_amd import ops
    dw_now = _now(c, dev)
    q = ops.new_wgrad_queue()
    call = Call(c, dev).run(queue=q)
    torch.cuda.synchronize()
    if c.co * c.ci % 4 != 0:                    # the batched kernel moves 16 bytes: such a layer is reduced at once
        assert q.pending() == 0
    else:
        assert q.pending() == 1
        assert WC.all_pattern(call.dw), 'the queued call already wrote dw'
        _flush(q)
        assert q.pending() == 0
    assert _bits_equal(call.dw, dw_now) and call.guards_intact()


@pytest.mark.parametrize('order', ('table', 'reversed'))
def test_one_flush_over_mixed_layers(dev, order):
    from aide_amd import ops
    cases = list(WC.CASES) if order == 'table' else list(reversed(WC.CASES))
    now = [_now(c, dev) for c in cases]
    q = ops.new_wgrad_queue()
    calls = [Call(c, dev).run(queue=q) for c in cases]
    queued = sum(1 for c in cases if c.co * c.ci % 4 == 0)
    assert q.pending() == queued and 16 < queued <= 48          # one launch of the batched kernel over every layer
    _flush(q)
    for c, call, ref in zip(cases, calls, now):
        assert _bits_equal(call.dw, ref), WC.case_id(c)
        assert call.guards_intact(), WC.case_id(c)


@pytest.fixture(scope='module')
def boundary(dev):
    """513 distinct inputs of the smallest summing case, their immediate results (computed once) and float64 references of a
    few of them"""
    c = WC.BOUNDARY_CASE
    assert c.n == 1
    g = torch.Generator().manual_seed(513)
    x = torch.randn(513, c.ci, c.h, c.w, generator=g)
    dz = torch.randn(513, c.co, c.h, c.w, generator=g)
    xd, dzd = x.to(dev), dz.to(dev)
    ops_ = [(dzd[i:i + 1], xd[i:i + 1]) for i in range(513)]
    now = []
    for i in range(513):
        call = Call(c, dev, operands=ops_[i]).run()
        now.append(call.dw)
    torch.cuda.synchronize()
    for i in (0, 47, 48, 96, 512):
        err = WC.rel_err(now[i].cpu().view(c.co, c.ci, 3, 3), WC.reference_dw(x[i:i + 1], dz[i:i + 1]))
        assert err <= WC.TOL[c.family], (i, err)
    return c, ops_, now


@pytest.mark.parametrize('count', (47, 48, 49, 97, 513))
def test_batch_boundaries(dev, boundary, count):
    """RB_MAX = 48 descriptors per launch of the batched kernel: one short of it, exactly it, one and two launches more.
    513: the handle holds 512 descriptors, so the last entry is reduced at once and the flush covers the other 512."""
    from aide_amd import ops
    c, operands, now = boundary
    q = ops.new_wgrad_queue()
    calls = [Call(c, dev, operands=operands[i]).run(queue=q) for i in range(count)]
    assert q.pending() == min(count, 512)
    torch.cuda.synchronize()
    assert all(WC.all_pattern(calls[i].dw) for i in (0, 46, min(count, 512) - 1))
    if count > 512:
        assert _bits_equal(calls[512].dw, now[512])         # already final
    _flush(q)
    assert q.pending() == 0
    for i, call in enumerate(calls):
        assert _bits_equal(call.dw, now[i]), i
        assert call.guards_intact(), i


def test_discard(dev, boundary):
    from aide_amd import ops
    c, operands, now = boundary
    q = ops.new_wgrad_queue()
    calls = [Call(c, dev, operands=operands[i]).run(queue=q) for i in range(3)]
    assert q.pending() == 3
    assert q.discard() == 3 and q.pending() == 0
    _flush(q)                                   # nothing pending: launches nothing
    assert all(WC.all_pattern(call.dw) and call.guards_intact() for call in calls)
    call = Call(c, dev, operands=operands[3]).run(queue=q)          # the queue is usable again
    assert q.pending() == 1
    _flush(q)
    assert _bits_equal(call.dw, now[3]) and call.guards_intact()
    assert all(WC.all_pattern(k.dw) for k in calls)
