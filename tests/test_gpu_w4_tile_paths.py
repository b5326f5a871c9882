"""Every prologue / epilogue path of the F(4x4) kernels (conv3x3_wino4.hip, conv3x3_wgrad4.hip) at the smallest shape that
reaches it (-m gpu): the three tile modes, the trailing half co block (whose guards are buffer range checks), the statistics
sink, accumulate, split-K with and without the reduce launch, the folded scale / bias / ReLU epilogue, the BatchNorm + ReLU
loader, and the weight gradient's odd chunk count / ragged column block / trailing half tile.

Reference: torch.nn.functional.conv2d in float64 on the CPU, bound 1e-4 of the output scale (the bound test_gpu_kernels.py
holds the F(4x4) kernels to).  On top of that, exact identities (torch.equal): the output with a bias is the output without
it plus bias[c] (one fp32 add per element), a statistics sink does not change the output, two launches into fresh buffers
agree bit for bit.

Statistics partials: a partial is the fp32 sum of the <= 512 pre-bias outputs (32 tiles x 16 pixels) of one (channel,
workgroup tile), resp. of their squares (fmaf chain).  Against the float64 sums of the SAME device outputs the error of an
fp32 sum of n terms in any order is at most (n - 1) u sum|t| (u = 2^-24), one more u for the square itself: the bound used is
512 * 2^-24 * sum|y| and 513 * 2^-24 * sum y^2 per partial."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _close(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    assert err <= 1e-4 * scale, '%s: max abs err %.3e > %.3e (ref scale %.3e)' % (what, err, 1e-4 * scale, scale)


def _tiles(h, w):
    """(mode, tile height, tile width, tiles down, tiles across) of a plane: the library's rule (f4_mode of conv3x3_wino4.hip)"""
    sh, sw, ch, cw = (h + 15) // 16, (w + 31) // 32, (h + 19) // 20, (w + 19) // 20
    if w == 16:
        return 1, 16, 32, sh, sw
    if ch * cw < sh * sw:
        return 2, 20, 20, ch, cw
    return 0, 16, 32, sh, sw


@functools.lru_cache(maxsize=None)
def _problem(n, ci, co, h, w):
    """inputs and the float64 reference of one shape, computed once and shared (never modified)"""
    g = torch.Generator().manual_seed(1000 * ci + 10 * co + h + w)
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, 3, 3, generator=g) * (1.0 / (3.0 * ci ** 0.5))
    b = torch.randn(co, generator=g)
    dy = torch.randn(n, co, h, w, generator=g)
    xr = x.double().requires_grad_(True)
    wr = wt.double().requires_grad_(True)
    y = F.conv2d(xr, wr, None, padding=1)
    y.backward(dy.double())
    return dict(x=x, w=wt, b=b, dy=dy, y=y.detach(), dx=xr.grad, dw=wr.grad)


def _fwd(ops, dev, p, bias=None, stats=False, **kw):
    """one launch into a fresh (poisoned) buffer -> (y, statistics partials | None)"""
    x = p['x'].to(dev)
    co = p['w'].shape[0]
    n, _, h, w = x.shape
    uf, _ = ops.wino4_pack(p['w'].to(dev), need_dgrad=False)
    y = torch.full((n, co, h, w), 3.0, device=dev)
    st = None
    if stats:
        from aide_amd._lib import lib
        parts = lib.aide_conv3x3_wino4_stats_parts(n, h, w)
        assert parts > 0
        st = torch.full((co * parts * 2,), float('nan'), device=dev)
    ops.conv3x3_wino4(x, uf, None if bias is None else bias.to(dev), y, stats=st, **kw)
    return y, st


def _identities(ops, dev, p, what, stats_ok, **kw):
    """reference + the exact identities of a forward shape; returns the pre-bias device output"""
    b = p['b']
    y0, _ = _fwd(ops, dev, p, **kw)
    _close(y0, p['y'], what + ' no bias')
    yb, _ = _fwd(ops, dev, p, bias=b, **kw)
    _close(yb, p['y'] + b.double().view(1, -1, 1, 1), what + ' bias')
    assert torch.equal(yb, y0 + b.to(dev).view(1, -1, 1, 1)), what + ': bias is not one fp32 add on the output without it'
    assert torch.equal(_fwd(ops, dev, p, bias=b, **kw)[0], yb), what + ': two launches differ'
    if stats_ok:
        ys, st = _fwd(ops, dev, p, bias=b, stats=True, **kw)
        assert torch.equal(ys, yb), what + ': the statistics sink changes the output'
        _check_stats(st, y0, what)
    return y0


def _check_stats(st, y0, what):
    n, co, h, w = y0.shape
    mode, th, tw, bh, bw = _tiles(h, w)
    assert mode != 1
    st = st.view(co, n * bh * bw, 2).cpu().double()
    y = y0.cpu().double()
    for img in range(n):
        for i in range(bh):
            for j in range(bw):
                t = y[img, :, i * th:(i + 1) * th, j * tw:(j + 1) * tw].reshape(co, -1)
                blk = (img * bh + i) * bw + j
                s1, s2, sa = t.sum(1), (t * t).sum(1), t.abs().sum(1)
                e1 = (st[:, blk, 0] - s1).abs() - 512 * U * sa
                e2 = (st[:, blk, 1] - s2).abs() - 513 * U * s2
                assert e1.max().item() <= 0 and e2.max().item() <= 0, \
                    '%s: statistics partial of tile %d off by %.3e / %.3e beyond the bound' % (what, blk, e1.max().item(), e2.max().item())


# ---- 1, 3: MODE 0, one exact tile and ragged tiles, with and without bias, with and without the statistics sink ----
@pytest.mark.parametrize('hw', [(16, 32), (20, 36)])
def test_plain_tiles_bias_and_statistics(dev, hw):
    from aide_amd import ops
    p = _problem(2, 8, 64, *hw)
    _identities(ops, dev, p, 'wino4 8->64 %dx%d' % hw, stats_ok=True)


# ---- 2: trailing half co block: the bias loads and the stores of the upper 32 rows are range-checked away ----
def test_trailing_half_co_block(dev):
    from aide_amd import ops
    p = _problem(2, 8, 96, 16, 32)
    n, co, h, w = 2, 96, 16, 32
    # the output sits in the middle of a larger buffer: rows past Cout must not be written
    x = p['x'].to(dev)
    uf, _ = ops.wino4_pack(p['w'].to(dev), need_dgrad=False)
    big = torch.full((n, co + 64, h, w), 5.0, device=dev)
    y = big[:, :co]
    ops.conv3x3_wino4(x, uf, p['b'].to(dev), y)
    _close(y, p['y'] + p['b'].double().view(1, -1, 1, 1), 'wino4 8->96 in a wider buffer')
    assert (big[:, co:] == 5.0).all().item(), 'rows past Cout were written'
    _identities(ops, dev, p, 'wino4 8->96 16x32', stats_ok=True)


# ---- 4: accumulate = 1 onto random contents ----
def test_accumulate(dev):
    from aide_amd import ops
    p = _problem(2, 16, 64, 16, 32)
    g = torch.Generator().manual_seed(5)
    old = torch.randn(2, 64, 16, 32, generator=g)
    uf, _ = ops.wino4_pack(p['w'].to(dev), need_dgrad=False)
    outs = []
    for _ in range(2):
        y = old.to(dev).clone()
        ops.conv3x3_wino4(p['x'].to(dev), uf, None, y, accumulate=True)
        outs.append(y)
    _close(outs[0], p['y'] + old.double(), 'wino4 accumulate')
    assert torch.equal(outs[0], outs[1]), 'two accumulate launches differ'
    y0, _ = _fwd(ops, dev, p)
    assert torch.equal(outs[0], y0 + old.to(dev)), 'accumulate is not one fp32 add of the old contents'


# ---- 5: split-K: the reduce launch, accumulate = 2 slabs, and the data gradient (64 -> 64 has a dgrad pack) ----
def test_splitk_reduce_and_slabs(dev):
    from aide_amd import ops
    from aide_amd._lib import lib
    n, ci, co, h, w = 2, 64, 64, 32, 32
    p = _problem(n, ci, co, h, w)
    sk = lib.aide_conv3x3_wino4_splitk(n, ci, h, w, co)
    assert sk > 1
    y0 = _identities(ops, dev, p, 'wino4 split-K %d' % sk, stats_ok=False, splitk=sk)
    assert torch.equal(_fwd(ops, dev, p)[0], y0), 'the library-chosen split is not the queried one'
    _close(_fwd(ops, dev, p, splitk=1)[0], p['y'], 'wino4 64->64 unsplit')
    uf, ud = ops.wino4_pack(p['w'].to(dev), need_dgrad=True)
    slabs = torch.full((sk * n * co * h * w,), float('nan'), device=dev)
    ops.conv3x3_wino4(p['x'].to(dev), uf, None, torch.empty(n, co, h, w, device=dev), accumulate=2, splitk=sk, ws=slabs)
    sl = slabs.view(sk, n, co, h, w)
    acc = sl[0].clone()
    for s in range(1, sk):
        acc += sl[s]                                       # the order of the reduce
    assert torch.equal(acc, y0), 'slabs summed in split order differ from the reduced output'
    dxs = []
    for _ in range(2):
        dx = torch.ones(n, ci, h, w, device=dev)
        ops.conv3x3_wino4(p['dy'].to(dev), ud, None, dx, accumulate=True)
        dxs.append(dx)
    _close(dxs[0], p['dx'] + 1.0, 'wino4 dgrad accumulate')
    assert torch.equal(dxs[0], dxs[1]), 'two dgrad launches differ'


# ---- 6: MODE 1, two 16-wide images per workgroup tile ----
def test_image_pair_tile(dev):
    from aide_amd import ops
    assert _tiles(16, 16)[0] == 1
    p = _problem(2, 8, 64, 16, 16)
    _identities(ops, dev, p, 'wino4 pair tile', stats_ok=False)


# ---- 7: MODE 2, the 20 x 20 canvas: one tile, four tiles ----
@pytest.mark.parametrize('hw', [(20, 20), (40, 40)])
def test_canvas_tile(dev, hw):
    from aide_amd import ops
    assert _tiles(*hw)[0] == 2
    p = _problem(1, 8, 64, *hw)
    _identities(ops, dev, p, 'wino4 canvas %dx%d' % hw, stats_ok=hw[1] >= 32)


# ---- 8: AFF epilogue y = relu?(acc * scale + bias) on the plain and the canvas tile ----
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('shape', [(2, 16, 32), (2, 20, 36), (1, 20, 20), (1, 40, 40)])
def test_folded_scale_bias_relu(dev, shape, relu):
    from aide_amd import ops
    n, h, w = shape
    p = _problem(n, 8, 64, h, w)
    g = torch.Generator().manual_seed(h + w)
    sc = torch.randn(64, generator=g)                      # both signs
    ref = p['y'] * sc.double().view(1, -1, 1, 1) + p['b'].double().view(1, -1, 1, 1)
    if relu:
        ref = ref.clamp_min(0.0)
    ya, _ = _fwd(ops, dev, p, bias=p['b'], epi_scale=sc.to(dev), epi_relu=relu)
    # (the bound is relative to the scale of the pre-activation: the ReLU only removes values)
    _close(ya, ref, 'wino4 folded epilogue relu=%s %s' % (relu, shape))
    assert torch.equal(_fwd(ops, dev, p, bias=p['b'], epi_scale=sc.to(dev), epi_relu=relu)[0], ya), 'two launches differ'


# ---- 9: BNIN loader: relu(x * scale + shift) per image group on the way in ----
@pytest.mark.parametrize('groups', [1, 2])
def test_input_batchnorm_loader(dev, groups):
    from aide_amd import ops
    n, ci, co, h, w = 2, 8, 64, 16, 32
    p = _problem(n, ci, co, h, w)
    g = torch.Generator().manual_seed(groups)
    tab = torch.randn(groups, ci, 2, generator=g)          # (scale, shift): both signs -- BN(0) != 0, the halo must stay 0
    ng = n // groups
    act = torch.empty(n, ci, h, w, dtype=torch.float64)
    for gi in range(groups):
        sl = slice(gi * ng, (gi + 1) * ng)
        act[sl] = (p['x'][sl].double() * tab[gi, :, 0].double().view(1, ci, 1, 1) + tab[gi, :, 1].double().view(1, ci, 1, 1)).clamp_min(0.0)
    ref = F.conv2d(act, p['w'].double(), None, padding=1)
    kw = dict(in_tab=tab.to(dev), in_group_images=ng)
    y0, _ = _fwd(ops, dev, p, **kw)
    _close(y0, ref, 'wino4 input BatchNorm, %d group(s)' % groups)
    yb, _ = _fwd(ops, dev, p, bias=p['b'], **kw)
    assert torch.equal(yb, y0 + p['b'].to(dev).view(1, -1, 1, 1)), 'bias is not one fp32 add on the output without it'
    ys, st = _fwd(ops, dev, p, bias=p['b'], stats=True, **kw)
    assert torch.equal(ys, yb), 'the statistics sink changes the output'
    _check_stats(st, y0, 'wino4 input BatchNorm')
    assert torch.equal(_fwd(ops, dev, p, bias=p['b'], **kw)[0], yb), 'two launches differ'


# ---- 10, 11: weight gradient: odd chunk count + ragged last column block; trailing half tile (Co % 64 == 32) ----
@pytest.mark.parametrize('case', [(1, 64, 32, 20, 20), (1, 32, 32, 16, 16)])
def test_weight_gradient_tile_paths(dev, case):
    from aide_amd import ops
    n, co, ci, h, w = case
    assert ops.wgrad_wino4_supported(co, ci, h, w)
    p = _problem(n, ci, co, h, w)
    from aide_amd._lib import lib
    dyd, xd = p['dy'].to(dev), p['x'].to(dev)
    # target 0: the library's split; 4: three chunks per split (an odd count: the pair loop runs one chunk past the end)
    for target in (0, 4):
        nws = lib.aide_conv3x3_wgrad_wino4_ws_bytes_t(n, co, ci, h, w, target) // 4
        ws = torch.full((nws + 4096,), 5.0, device=dev)    # slabs + a guard region: rows past Co must not be written
        dw = ops.conv3x3_wgrad_wino4(dyd, xd, torch.empty(co, ci, 3, 3, device=dev), ws=ws[:nws], target_wgs=target)
        _close(dw, p['dw'], 'wino4 wgrad %s target %d' % (case, target))
        assert (ws[nws:] == 5.0).all().item(), 'the slab stores ran past the workspace'
        dw2 = ops.conv3x3_wgrad_wino4(dyd, xd, torch.empty(co, ci, 3, 3, device=dev), target_wgs=target)
        assert torch.equal(dw2, dw), 'two launches differ'
