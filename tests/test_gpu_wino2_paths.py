"""Every prologue / main-loop / epilogue path of the F(2x2) Winograd kernel (conv3x3_winograd.hip) at the smallest shape that
reaches it (-m gpu): chunk counts that end in the prologue, on either stage set and on an odd count; uneven split-K ranges
with and without the reduce launch; two co tiles, ragged tile rows and columns, three images, bias present and absent,
accumulate onto non-zero contents -- all of them on channel slices of wider, NaN-filled buffers, so that a store or a load that
strays from its descriptor shows.

Reference: torch.nn.functional.conv2d in float64 on the CPU; bound: 2e-5 of the output scale, the bound test_gpu_kernels.py
holds this family to."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _close(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    assert err <= 2e-5 * scale, '%s: max abs err %.3e > %.3e (ref scale %.3e)' % (what, err, 2e-5 * scale, scale)


@functools.lru_cache(maxsize=None)
def _problem(n, ci, co, h, w):
    """inputs and the float64 reference (without bias) of one shape, computed once and shared (never modified)"""
    g = torch.Generator().manual_seed(1000 * ci + 10 * co + h + w)
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, 3, 3, generator=g) * (1.0 / (3.0 * ci ** 0.5))
    b = torch.randn(co, generator=g)
    old = torch.randn(n, co, h, w, generator=g)
    y = F.conv2d(x.double(), wt.double(), None, padding=1)
    return dict(x=x, w=wt, b=b, old=old, y=y)


def _bias64(p):
    return p['b'].double().view(1, -1, 1, 1)


def _launch(ops, dev, p, bias=False, **kw):
    """one launch into a fresh (poisoned) dense buffer"""
    n, co, h, w = p['y'].shape
    uf, _ = ops.wino_pack(p['w'].to(dev), need_dgrad=False)
    y = torch.full((n, co, h, w), 3.0, device=dev)
    ops.conv3x3_wino(p['x'].to(dev), uf, p['b'].to(dev) if bias else None, y, **kw)
    return y


# ---- chunk counts: 1 (the prologue only), 2 and 3 (both stage sets), 9 (odd, several loop rounds) ----
@pytest.mark.parametrize('ci', [8, 16, 24, 72])
def test_chunk_counts(dev, ci):
    from aide_amd import ops
    assert ops.wino_supported(ci, 16, 16, 64)
    p = _problem(1, ci, 64, 16, 16)
    y = _launch(ops, dev, p, bias=True, splitk=1)
    _close(y, p['y'] + _bias64(p), 'wino %d chunks' % (ci // 8))
    assert torch.equal(_launch(ops, dev, p, bias=True, splitk=1), y), 'two launches differ'


# ---- split-K on five chunks: ranges 3 + 2 and 2 + 2 + 1; reduced by the library, and as slabs (accumulate = 2) ----
@pytest.mark.parametrize('splitk', [2, 3])
def test_splitk_uneven_ranges(dev, splitk):
    from aide_amd import ops
    from aide_amd._lib import lib
    n, ci, co, h, w = 1, 40, 64, 16, 16
    p = _problem(n, ci, co, h, w)
    y = _launch(ops, dev, p, splitk=splitk)
    _close(y, p['y'], 'wino split-K %d reduced' % splitk)
    yb = _launch(ops, dev, p, bias=True, splitk=splitk)
    _close(yb, p['y'] + _bias64(p), 'wino split-K %d reduced, bias' % splitk)
    nws = lib.aide_conv3x3_ws_bytes(n, h, w, co, splitk) // 4
    assert nws >= splitk * n * co * h * w
    slabs = torch.full((nws,), float('nan'), device=dev)
    uf, _ = ops.wino_pack(p['w'].to(dev), need_dgrad=False)
    out = torch.full((n, co, h, w), 3.0, device=dev)
    ops.conv3x3_wino(p['x'].to(dev), uf, None, out, accumulate=2, splitk=splitk, ws=slabs)
    assert (out == 3.0).all().item(), 'accumulate = 2 wrote the output'
    sl = slabs[:splitk * n * co * h * w].view(splitk, n, co, h, w)
    acc = sl[0].clone()
    for s in range(1, splitk):
        acc += sl[s]                                       # the order of the reduce
    assert torch.equal(acc, y), 'slabs summed in split order differ from the reduced output'


# ---- epilogue guards: two co tiles, ragged tile rows / columns, three images, on slices of NaN-filled buffers ----
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('hw', [(6, 12), (18, 20), (34, 36)])
def test_epilogue_guards_on_slices(dev, hw, bias, accumulate):
    from aide_amd import ops
    n, ci, co = 3, 16, 128
    h, w = hw
    assert ops.wino_supported(ci, h, w, co)
    p = _problem(n, ci, co, h, w)
    nan = float('nan')
    # channel slices in the middle of wider buffers (extra channels before and after: batch stride > C * H * W)
    xbig = torch.full((n, ci + 12, h, w), nan, device=dev)
    ybig = torch.full((n, co + 8, h, w), nan, device=dev)
    xs, ys = xbig[:, 4:4 + ci], ybig[:, 4:4 + co]
    xs.copy_(p['x'])
    ref = p['y'].clone()
    if bias:
        ref += _bias64(p)
    if accumulate:
        ys.copy_(p['old'])
        ref += p['old'].double()
    uf, _ = ops.wino_pack(p['w'].to(dev), need_dgrad=False)
    ops.conv3x3_wino(xs, uf, p['b'].to(dev) if bias else None, ys, accumulate=accumulate, splitk=1)
    what = 'wino 16->128 %dx%d bias=%s accumulate=%s' % (h, w, bias, accumulate)
    assert not torch.isnan(ys).any().item(), what + ': NaN in the output'
    _close(ys, ref, what)
    assert torch.isnan(ybig[:, :4]).all().item() and torch.isnan(ybig[:, 4 + co:]).all().item(), \
        what + ': channels outside the output slice were written'
    assert torch.isnan(xbig[:, :4]).all().item() and torch.isnan(xbig[:, 4 + ci:]).all().item(), \
        what + ': the input buffer was written'
    # the same launch again, from the same contents: bit-identical
    y2big = torch.full((n, co + 8, h, w), nan, device=dev)
    y2 = y2big[:, 4:4 + co]
    if accumulate:
        y2.copy_(p['old'])
    ops.conv3x3_wino(xs, uf, p['b'].to(dev) if bias else None, y2, accumulate=accumulate, splitk=1)
    assert torch.equal(y2, ys), what + ': two launches differ'


# ---- the exact identities of the epilogue: bias and the old contents are one fp32 add each ----
def test_bias_and_accumulate_are_single_adds(dev):
    from aide_amd import ops
    p = _problem(3, 16, 128, 18, 20)
    y0 = _launch(ops, dev, p)
    yb = _launch(ops, dev, p, bias=True)
    assert torch.equal(yb, y0 + p['b'].to(dev).view(1, -1, 1, 1)), 'bias is not one fp32 add on the output without it'
    uf, _ = ops.wino_pack(p['w'].to(dev), need_dgrad=False)
    ya = p['old'].to(dev).clone()
    ops.conv3x3_wino(p['x'].to(dev), uf, None, ya, accumulate=True, splitk=1)
    assert torch.equal(ya, (y0 + 0.0) + p['old'].to(dev)), 'accumulate is not one fp32 add of the old contents'


# ---- the data-gradient pack (rotated, channel-transposed filters) through the same kernel, split by the library's rule ----
def test_dgrad_pack_accumulate(dev):
    from aide_amd import ops
    n, ci, co, h, w = 1, 64, 128, 16, 16
    g = torch.Generator().manual_seed(7)
    wt = torch.randn(co, ci, 3, 3, generator=g) * (1.0 / (3.0 * ci ** 0.5))
    x = torch.randn(n, ci, h, w, generator=g)
    dy = torch.randn(n, co, h, w, generator=g)
    xr = x.double().requires_grad_(True)
    yr = F.conv2d(xr, wt.double(), None, padding=1)
    yr.backward(dy.double())
    uf, ud = ops.wino_pack(wt.to(dev), need_dgrad=True)
    y = torch.full((n, co, h, w), 3.0, device=dev)
    ops.conv3x3_wino(x.to(dev), uf, None, y)
    _close(y, yr, 'wino 64->128 forward pack')
    dxs = []
    for _ in range(2):
        dx = torch.ones(n, ci, h, w, device=dev)
        ops.conv3x3_wino(dy.to(dev), ud, None, dx, accumulate=True)
        dxs.append(dx)
    _close(dxs[0], xr.grad + 1.0, 'wino 128->64 data-gradient pack, accumulate')
    assert torch.equal(dxs[0], dxs[1]), 'two data-gradient launches differ'
