"""bf16-MFMA conv mode (-m gpu; BASELINE config 5).  Contract (aide_amd/csrc/conv3x3_bf16.hip): operands are rounded
to bf16 (RNE) when staged, products accumulate in fp32.  The check is therefore two-sided:
  * tight: against the aten fp32 convolution of the bf16-ROUNDED operands (what the kernel computes, up to fp32
    summation order) -- tolerance 3e-5 of the output scale;
  * loose: against the plain fp32 convolution of the unrounded operands -- the bf16 input-rounding bound
    (2^-8 relative per operand, random signs): 1e-2 of the output scale.
The packed filters are compared bit-exactly with torch's RNE bf16 conversion."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rb(t):
    return t.bfloat16().float()


def _close(got, ref, rtol, what=''):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    assert err <= rtol * scale, '%s: max abs err %.3e > %.3e (ref scale %.3e)' % (what, err, rtol * scale, scale)


def test_bf16_pack_bit_exact(dev):
    from aide_amd import ops
    g = torch.Generator().manual_seed(5)
    for co, ci in ((32, 3), (64, 40), (128, 64)):
        w = torch.randn(co, ci, 3, 3, generator=g)
        uf, ud = ops.bf16_pack(w.to(dev))
        torch.cuda.synchronize()
        cf, cd = (ci + 15) // 16, (co + 15) // 16
        wb = w.bfloat16().view(torch.int16)                      # [co][ci][3][3] bit patterns
        ref_f = torch.zeros(cf * 16, 9, co, dtype=torch.int16)
        ref_f[:ci] = wb.reshape(co, ci, 9).permute(1, 2, 0)
        ref_f = ref_f.view(cf, 2, 8, 9, co).permute(0, 3, 1, 4, 2).contiguous()      # [chunk][tap][g][co][8]
        assert torch.equal(uf.cpu().view(cf, 9, 2, co, 8), ref_f), 'forward pack %dx%d' % (co, ci)
        ref_d = torch.zeros(cd * 16, 9, ci, dtype=torch.int16)
        ref_d[:co] = wb.reshape(co, ci, 9).flip(2).permute(0, 2, 1)
        ref_d = ref_d.view(cd, 2, 8, 9, ci).permute(0, 3, 1, 4, 2).contiguous()
        assert torch.equal(ud.cpu().view(cd, 9, 2, ci, 8), ref_d), 'dgrad pack %dx%d' % (co, ci)


BF16_CASES = [
    # N, Cin, Cout, H, W
    (2, 3, 32, 32, 32), (1, 32, 32, 64, 64), (2, 64, 64, 32, 32), (1, 128, 64, 64, 64), (2, 64, 128, 16, 32),
    (1, 256, 256, 32, 32), (1, 40, 96, 24, 64), (2, 512, 512, 32, 32), (1, 32, 64, 20, 96),
    (1, 64, 64, 24, 128), (1, 3, 32, 12, 192),          # 64-column tiles (W >= 128), ragged bottom rows
]


@pytest.mark.parametrize('case', BF16_CASES)
def test_conv3x3_bf16_fwd_dgrad(dev, case):
    from aide_amd import ops
    n, ci, co, h, w = case
    assert ops.bf16_supported(ci, h, w, co)
    g = torch.Generator().manual_seed(ci * 131 + co)
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, 3, 3, generator=g) * (1.0 / (3.0 * ci ** 0.5))
    b = torch.randn(co, generator=g)
    dy = torch.randn(n, co, h, w, generator=g)
    y_exact = F.conv2d(_rb(x), _rb(wt), b, padding=1)
    y_fp32 = F.conv2d(x, wt, b, padding=1)
    dx_exact = F.conv_transpose2d(_rb(dy), _rb(wt), padding=1)
    dx_fp32 = F.conv_transpose2d(dy, wt, padding=1)

    xd, wd_, bd, dyd = x.to(dev), wt.to(dev), b.to(dev), dy.to(dev)
    uf, ud = ops.bf16_pack(wd_, need_dgrad=(ci % 32 == 0))
    for splitk in (1, 2, 4):
        if splitk > (ci + 15) // 16:
            continue
        y = torch.full((n, co, h, w), float('nan'), device=dev)
        ops.conv3x3_bf16(xd, uf, bd, y, splitk=splitk)
        _close(y, y_exact, 3e-5, 'fwd exact splitk %d %s' % (splitk, case))
        _close(y, y_fp32, 1e-2, 'fwd vs fp32 splitk %d %s' % (splitk, case))
    if ud is not None:
        for splitk in (1, 2):
            base = torch.randn(n, ci, h, w, generator=g)
            dx = base.to(dev)
            ops.conv3x3_bf16(dyd, ud, None, dx, accumulate=True, splitk=splitk)       # skip-connection form
            _close(dx, dx_exact + base, 3e-5, 'dgrad exact splitk %d %s' % (splitk, case))
            _close(dx, dx_fp32 + base, 1e-2, 'dgrad vs fp32 %s' % (case,))


def test_bf16_storage_variants(dev):
    """z stored as bf16 by the forward (= RNE of the fp32-output kernel's result, bit for bit), dz read as bf16 by the
    dgrad / wgrad (= the fp32-input kernels on the widened values, bit for bit), with and without split-K."""
    from aide_amd import ops
    g = torch.Generator().manual_seed(21)
    for (n, ci, co, h, w) in ((2, 64, 64, 32, 32), (1, 3, 32, 20, 64), (1, 128, 96, 16, 32), (1, 32, 64, 12, 128)):
        x = torch.randn(n, ci, h, w, generator=g).to(dev)
        wt = (torch.randn(co, ci, 3, 3, generator=g) * 0.1).to(dev)
        b = torch.randn(co, generator=g).to(dev)
        uf, ud = ops.bf16_pack(wt, need_dgrad=(ci % 32 == 0))
        for splitk in (1, 2):
            if splitk > (ci + 15) // 16:
                continue
            y32 = torch.empty(n, co, h, w, device=dev)
            ops.conv3x3_bf16(x, uf, b, y32, splitk=splitk)
            y16 = torch.empty(n, co, h, w, device=dev, dtype=torch.bfloat16)
            ops.conv3x3_bf16(x, uf, b, y16, splitk=splitk)
            assert torch.equal(y16, y32.bfloat16()), 'bf16 z, splitk %d, %s' % (splitk, (n, ci, co, h, w))
        if ud is not None:
            dz16 = torch.randn(n, co, h, w, generator=g).to(dev).bfloat16()
            dx_a, dx_b = torch.empty(n, ci, h, w, device=dev), torch.empty(n, ci, h, w, device=dev)
            ops.conv3x3_bf16(dz16, ud, None, dx_a)
            ops.conv3x3_bf16(dz16.float(), ud, None, dx_b)
            assert torch.equal(dx_a, dx_b), 'bf16 dz dgrad'
            if ops.wgrad_bf16_supported(co, ci, h, w):
                dw_a, dw_b = torch.empty_like(wt), torch.empty_like(wt)
                ops.conv3x3_wgrad_bf16(dz16, x, dw_a)
                ops.conv3x3_wgrad_bf16(dz16.float(), x, dw_b)
                assert torch.equal(dw_a, dw_b), 'bf16 dz wgrad'


@pytest.mark.parametrize('shape', [(2, 32, 32, 32), (4, 64, 16, 16), (1, 8, 6, 5),
                                   (8, 1, 514, 514)])        # (two passes, 4 wide, whatever the storage)
def test_bn_on_bf16_storage(dev, shape):
    """BatchNorm forward / backward on a bf16-stored z and into a bf16-stored dz: bit-identical to the fp32-storage
    kernels on the widened z, with dz narrowed RNE."""
    from aide_amd import ops
    n, c, h, w = shape
    g = torch.Generator().manual_seed(c)
    z16 = torch.randn(n, c, h, w, generator=g).to(dev).bfloat16()
    dA = torch.randn(n, c, h, w, generator=g).to(dev)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
    res = []
    for z in (z16, z16.float()):
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        nbt = torch.zeros((), dtype=torch.long, device=dev)
        st = [torch.empty(c, device=dev) for _ in range(4)]
        a = torch.empty(n, c, h, w, device=dev)
        ws = ops.bn_ws(c, dev)
        ops.bn_train_fwd(z, a, gamma, beta, 1e-5, 0.1, rm, rv, nbt, st[0], st[1], st[2], st[3], ws, True)
        dz = torch.empty(n, c, h, w, device=dev, dtype=z.dtype)
        dg, db, dbias = torch.empty(c, device=dev), torch.empty(c, device=dev), torch.empty(c, device=dev)
        ops.bn_relu_bwd(dA, z, dz, st[0], st[1], st[2], st[3], dg, db, dbias, ws, True)
        a_eval = torch.empty_like(a)
        ops.bn_relu_apply(z, a_eval, st[2], st[3], True)
        res.append((a, rm, rv, dz, dg, db, a_eval))
    for t16, t32 in zip(res[0], res[1]):
        if t16.dtype == torch.bfloat16:
            assert torch.equal(t16, t32.bfloat16())
        else:
            assert torch.equal(t16, t32)


def test_bf16_stored_activations(dev):
    """Every operator that touches a bf16-stored activation: result == the fp32-storage operator on the widened input,
    narrowed RNE where the output is bf16-stored (bit for bit; BatchNorm-apply, pooling, up-sampling, head, conv forward
    and weight gradient)."""
    from aide_amd import ops
    g = torch.Generator().manual_seed(33)
    n, c, h, w = 2, 64, 16, 64
    a16 = torch.randn(n, c, h, w, generator=g).to(dev).bfloat16()
    a32 = a16.float()
    # BatchNorm apply into a bf16 activation (train and eval form), from fp32 and bf16 z
    for z in (torch.randn(n, c, h, w, generator=g).to(dev), torch.randn(n, c, h, w, generator=g).to(dev).bfloat16()):
        outs = []
        for dt in (torch.bfloat16, torch.float32):
            rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
            nbt = torch.zeros((), dtype=torch.long, device=dev)
            st = [torch.empty(c, device=dev) for _ in range(4)]
            gam, bet = torch.ones(c, device=dev), torch.zeros(c, device=dev)
            a = torch.empty(n, c, h, w, device=dev, dtype=dt)
            ops.bn_train_fwd(z, a, gam, bet, 1e-5, 0.1, rm, rv, nbt, st[0], st[1], st[2], st[3], ops.bn_ws(c, dev), True)
            e = torch.empty(n, c, h, w, device=dev, dtype=dt)
            ops.bn_relu_apply(z, e, st[2], st[3], True)
            outs.append((a, e))
        assert torch.equal(outs[0][0], outs[1][0].bfloat16()) and torch.equal(outs[0][1], outs[1][1].bfloat16())
    # max-pool forward (all four storage combinations) and backward (arg-max from the bf16 tensor)
    ref = torch.empty(n, c, h // 2, w // 2, device=dev)
    ops.maxpool2x2_fwd(a32, ref)
    for dt in (torch.bfloat16, torch.float32):
        y = torch.empty(n, c, h // 2, w // 2, device=dev, dtype=dt)
        ops.maxpool2x2_fwd(a16, y)
        assert torch.equal(y.float(), ref)                       # the maximum of bf16 values is a bf16 value
    y16 = torch.empty(n, c, h // 2, w // 2, device=dev, dtype=torch.bfloat16)
    ops.maxpool2x2_fwd(a32 * 1.001, y16)
    ref2 = torch.empty_like(ref)
    ops.maxpool2x2_fwd(a32 * 1.001, ref2)
    assert torch.equal(y16, ref2.bfloat16())
    dy = torch.randn(n, c, h // 2, w // 2, generator=g).to(dev)
    dxa, dxb = torch.empty(n, c, h, w, device=dev), torch.empty(n, c, h, w, device=dev)
    ops.maxpool2x2_bwd(a16, dy, dxa)
    ops.maxpool2x2_bwd(a32, dy, dxb)
    assert torch.equal(dxa, dxb)
    # bilinear x2
    up_ref = torch.empty(n, c, 2 * h, 2 * w, device=dev)
    ops.upsample2x_fwd(a32, up_ref)
    for dt in (torch.bfloat16, torch.float32):
        u = torch.empty(n, c, 2 * h, 2 * w, device=dev, dtype=dt)
        ops.upsample2x_fwd(a16, u)
        # (the storage variants are separate template instantiations: the compiler may contract the interpolation
        # FMAs differently, so fp32 results agree to an ulp and the narrowed ones to a bf16 ulp on rounding ties)
        err = (u.float() - up_ref).abs()
        assert float((err - (2.0 ** -8 if dt == torch.bfloat16 else 1e-6) * up_ref.abs()).max()) <= 1e-6
    # head
    wh, bh = torch.randn(2, c, generator=g).to(dev), torch.randn(2, generator=g).to(dev)
    la, lb = torch.empty(n, 2, h, w, device=dev), torch.empty(n, 2, h, w, device=dev)
    ops.head1x1_fwd(a16, wh, bh, la)
    ops.head1x1_fwd(a32, wh, bh, lb)
    assert torch.equal(la, lb)
    dl = torch.randn(n, 2, h, w, generator=g).to(dev)
    gr = []
    for a in (a16, a32):
        dx, dw, db = torch.empty(n, c, h, w, device=dev), torch.empty(2, c, device=dev), torch.empty(2, device=dev)
        ops.head1x1_bwd(dl, a, wh, dx, dw, db)
        gr.append((dx, dw, db))
    assert all(torch.equal(p, q) for p, q in zip(*gr))
    # conv forward from a bf16-stored activation (into fp32 and bf16 z) and weight gradient reading it
    co = 64
    wt = (torch.randn(co, c, 3, 3, generator=g) * 0.05).to(dev)
    uf, _ = ops.bf16_pack(wt, need_dgrad=False)
    for dt in (torch.float32, torch.bfloat16):
        ya, yb = torch.empty(n, co, h, w, device=dev, dtype=dt), torch.empty(n, co, h, w, device=dev, dtype=dt)
        ops.conv3x3_bf16(a16, uf, None, ya)
        ops.conv3x3_bf16(a32, uf, None, yb)
        assert torch.equal(ya, yb), 'conv forward from bf16 activation, out %s' % dt
    for dz in (torch.randn(n, co, h, w, generator=g).to(dev), torch.randn(n, co, h, w, generator=g).to(dev).bfloat16()):
        dwa, dwb = torch.empty_like(wt), torch.empty_like(wt)
        ops.conv3x3_wgrad_bf16(dz, a16, dwa)
        ops.conv3x3_wgrad_bf16(dz, a32, dwb)
        assert torch.equal(dwa, dwb), 'wgrad from bf16 activation'
    # ... through channel slices of a wider bf16 buffer (concat buffers)
    big = torch.randn(n, c + 32, h, w, generator=g).to(dev).bfloat16()
    ya, yb = torch.empty(n, co, h, w, device=dev), torch.empty(n, co, h, w, device=dev)
    ops.conv3x3_bf16(big[:, 32:], uf, None, ya)
    ops.conv3x3_bf16(big[:, 32:].float().contiguous(), uf, None, yb)
    assert torch.equal(ya, yb)


def test_bf16_stored_activation_gradients(dev):
    """Operators that read / write / accumulate a bf16-stored activation gradient == the fp32-storage operators on the
    widened input, the result narrowed RNE once per write."""
    from aide_amd import ops
    g = torch.Generator().manual_seed(44)
    n, c, h, w = 2, 64, 16, 64
    x = torch.randn(n, c, h, w, generator=g).to(dev)
    # BatchNorm backward reading a bf16 dA
    z = torch.randn(n, c, h, w, generator=g).to(dev).bfloat16()
    dA16 = torch.randn(n, c, h, w, generator=g).to(dev).bfloat16()
    st = [torch.empty(c, device=dev) for _ in range(4)]
    gam, bet = torch.ones(c, device=dev), torch.zeros(c, device=dev)
    a = torch.empty(n, c, h, w, device=dev)
    ops.bn_train_fwd(z, a, gam, bet, 1e-5, 0.1, torch.zeros(c, device=dev), torch.ones(c, device=dev),
                     torch.zeros((), dtype=torch.long, device=dev), st[0], st[1], st[2], st[3], ops.bn_ws(c, dev), True)
    res = []
    for dA in (dA16, dA16.float()):
        dz = torch.empty(n, c, h, w, device=dev, dtype=torch.bfloat16)
        dg, db, dbias = (torch.empty(c, device=dev) for _ in range(3))
        ops.bn_relu_bwd(dA, z, dz, st[0], st[1], st[2], st[3], dg, db, dbias, ops.bn_ws(c, dev), True)
        res.append((dz, dg, db))
    assert all(torch.equal(p, q) for p, q in zip(*res))
    # max-pool backward: bf16 dy in, bf16 dx out, overwrite and accumulate
    dy16 = torch.randn(n, c, h // 2, w // 2, generator=g).to(dev).bfloat16()
    base16 = torch.randn(n, c, h, w, generator=g).to(dev).bfloat16()
    for acc in (False, True):
        d16, d32 = base16.clone(), base16.float()
        ops.maxpool2x2_bwd(x, dy16, d16, accumulate=acc)
        ops.maxpool2x2_bwd(x, dy16.float(), d32, accumulate=acc)
        assert torch.equal(d16, d32.bfloat16()), 'pool bwd accumulate=%s' % acc
    # up-sampling backward
    du16 = torch.randn(n, c, 2 * h, 2 * w, generator=g).to(dev).bfloat16()
    for acc in (False, True):
        d16, d32 = base16.clone(), base16.float()
        ops.upsample2x_bwd(du16, d16, accumulate=acc)
        ops.upsample2x_bwd(du16.float(), d32, accumulate=acc)
        err = (d16.float() - d32).abs() - 2.0 ** -8 * d32.abs()
        assert float(err.max()) <= 1e-6, 'upsample bwd accumulate=%s' % acc
    # head dgrad into a bf16 gradient buffer
    wh = torch.randn(2, c, generator=g).to(dev)
    dl = torch.randn(n, 2, h, w, generator=g).to(dev)
    dx16, dx32 = torch.empty(n, c, h, w, device=dev, dtype=torch.bfloat16), torch.empty(n, c, h, w, device=dev)
    dw, db = torch.empty(2, c, device=dev), torch.empty(2, device=dev)
    ops.head1x1_bwd(dl, x, wh, dx16, dw, db)
    ops.head1x1_bwd(dl, x, wh, dx32, dw, db)
    assert torch.equal(dx16, dx32.bfloat16())
    # conv dgrad: bf16 dz in, bf16 dA out, overwrite / accumulate, with and without split-K
    ci, co = 64, 128
    wt = (torch.randn(co, ci, 3, 3, generator=g) * 0.05).to(dev)
    _, ud = ops.bf16_pack(wt)
    dz16 = torch.randn(n, co, h, w, generator=g).to(dev).bfloat16()
    for splitk in (1, 2):
        for acc in (False, True):
            d16, d32 = base16.clone(), base16.float()
            ops.conv3x3_bf16(dz16, ud, None, d16, accumulate=acc, splitk=splitk)
            ops.conv3x3_bf16(dz16, ud, None, d32, accumulate=acc, splitk=splitk)
            assert torch.equal(d16, d32.bfloat16()), 'dgrad splitk=%d accumulate=%s' % (splitk, acc)
    # zero fill of a channel slice of a bf16 buffer
    buf = torch.ones(n, c + 32, h, w, device=dev, dtype=torch.bfloat16)
    ops.fill_zero(buf[:, 32:])
    assert float(buf[:, 32:].float().abs().max()) == 0.0 and float(buf[:, :32].float().min()) == 1.0


def test_conv3x3_bf16_channel_slices(dev):
    """inputs / outputs that are channel slices of concatenation buffers (explicit batch stride)."""
    from aide_amd import ops
    g = torch.Generator().manual_seed(9)
    n, ci, co, h, w = 2, 32, 64, 32, 32
    xbuf = torch.randn(n, ci + 16, h, w, generator=g)
    wt = torch.randn(co, ci, 3, 3, generator=g) * 0.05
    ybuf = torch.zeros(n, co + 32, h, w)
    yr = F.conv2d(_rb(xbuf[:, 16:]), _rb(wt), None, padding=1)
    xd, yd = xbuf.to(dev), ybuf.to(dev)
    uf, _ = ops.bf16_pack(wt.to(dev), need_dgrad=False)
    ops.conv3x3_bf16(xd[:, 16:], uf, None, yd[:, 32:])
    _close(yd[:, 32:], yr, 3e-5, 'slice fwd')
    assert float(yd[:, :32].abs().max()) == 0.0


WGRAD_CASES = [
    # N, Co, Ci, H, W
    (2, 32, 32, 32, 32), (1, 64, 64, 64, 64), (2, 64, 128, 16, 32), (1, 128, 64, 32, 96), (2, 256, 256, 32, 32),
    (1, 96, 32, 8, 64), (3, 64, 64, 4, 32), (2, 32, 3, 16, 64), (1, 64, 40, 8, 32),     # ragged input channels
    (1, 64, 3, 8, 128), (2, 96, 2, 4, 64), (2, 32, 3, 32, 32),       # stems: folded-tap kernel (W % 64 == 0) / general kernel
]


@pytest.mark.parametrize('case', [(2, 256, 256, 32, 32), (1, 128, 64, 32, 96), (1, 128, 40, 8, 32)])
def test_conv3x3_wgrad_bf16_wide_tile(dev, case):
    """the 128 co x 64 ci (8-wave) weight-gradient kernel, normally reserved for >= 150 GFLOP layers (co_blocks = 4)"""
    test_conv3x3_wgrad_bf16(dev, case, co_blocks=4)
    from aide_amd import ops
    n, co, ci, h, w = case
    g = torch.Generator().manual_seed(1)
    x16 = torch.randn(n, ci - ci % 8, h, w, generator=g).to(dev).bfloat16()
    dz16 = torch.randn(n, co, h, w, generator=g).to(dev).bfloat16()
    dw_wide = torch.empty(co, x16.shape[1], 3, 3, device=dev)
    ops.conv3x3_wgrad_bf16(dz16, x16, dw_wide, co_blocks=4)          # bf16-stored operands through the wide tile
    dw_ref = torch.empty_like(dw_wide)
    ops.conv3x3_wgrad_bf16(dz16, x16, dw_ref, co_blocks=2)
    _close(dw_wide, dw_ref, 2e-5, 'wide vs 64x64 tile %s' % (case,))


@pytest.mark.parametrize('case', [(2, 32, 32, 32, 32), (1, 32, 64, 8, 64), (2, 32, 40, 16, 32), (1, 64, 32, 16, 64), (2, 96, 24, 8, 32)])
def test_conv3x3_wgrad_bf16_narrow_tile(dev, case):
    """the 32 co x 64 ci (2-wave) tile of the 32-channel first-level layers (co_blocks = 1; the default for Co <= 32), also
    forced onto wider layers: several co tiles, a ci block that is skipped or partly masked"""
    test_conv3x3_wgrad_bf16(dev, case, co_blocks=1)
    from aide_amd import ops
    n, co, ci, h, w = case
    g = torch.Generator().manual_seed(3)
    x16 = torch.randn(n, ci - ci % 8, h, w, generator=g).to(dev).bfloat16()
    dz16 = torch.randn(n, co, h, w, generator=g).to(dev).bfloat16()
    dw1 = torch.empty(co, x16.shape[1], 3, 3, device=dev)
    ops.conv3x3_wgrad_bf16(dz16, x16, dw1, co_blocks=1)
    dw2 = torch.empty_like(dw1)
    ops.conv3x3_wgrad_bf16(dz16, x16, dw2, co_blocks=2)
    _close(dw1, dw2, 2e-5, '32-co vs 64x64 tile %s' % (case,))


@pytest.mark.parametrize('case', WGRAD_CASES)
def test_conv3x3_wgrad_bf16(dev, case, co_blocks=0):
    from aide_amd import ops
    n, co, ci, h, w = case
    assert ops.wgrad_bf16_supported(co, ci, h, w)
    g = torch.Generator().manual_seed(co * 17 + ci)
    x = torch.randn(n, ci, h, w, generator=g)
    dy = torch.randn(n, co, h, w, generator=g)

    def wgrad_ref(xx, dd):
        wt = torch.zeros(co, ci, 3, 3, requires_grad=True)
        F.conv2d(xx, wt, None, padding=1).backward(dd)
        return wt.grad
    dw_exact = wgrad_ref(_rb(x), _rb(dy))
    dw_fp32 = wgrad_ref(x, dy)
    dw = torch.full((co, ci, 3, 3), float('nan'), device=dev)
    ops.conv3x3_wgrad_bf16(dy.to(dev), x.to(dev), dw, co_blocks=co_blocks)
    _close(dw, dw_exact, 5e-5, 'wgrad exact %s' % (case,))
    _close(dw, dw_fp32, 1e-2, 'wgrad vs fp32 %s' % (case,))
    dw2 = torch.empty_like(dw)
    ops.conv3x3_wgrad_bf16(dy.to(dev), x.to(dev), dw2, co_blocks=co_blocks)
    assert torch.equal(dw, dw2), 'wgrad must be bit-reproducible'
    if ci <= 3:            # the stem layers read a bf16-STORED dz next to the fp32 image
        dw3 = torch.empty_like(dw)
        ops.conv3x3_wgrad_bf16(dy.to(dev).bfloat16(), x.to(dev), dw3)
        _close(dw3, dw_exact, 5e-5, 'wgrad, bf16-stored dz %s' % (case,))


# ------------------------------------------------------------------------------------------ whole network
def _pair(dev, kind='fuseunet', store=True):
    import oracle
    from oracle.bf16 import emulate_bf16
    from aide_amd.models_twomodalinputs import fuseunet
    from aide_amd.models_singlemodalinput import UNet
    ours_c, ref_c = (fuseunet, oracle.fuseunet) if kind == 'fuseunet' else (UNet, oracle.UNet)
    torch.manual_seed(2)
    ref = emulate_bf16(ref_c(2))
    torch.manual_seed(2)
    net = ours_c(2).to(dev)
    net.engine.precision = 'bf16'
    cfg = net.engine.config                      # the storage switches of THIS network's engine
    cfg.store_bf16 = cfg.store_a_bf16 = cfg.store_g_bf16 = store
    return net, ref


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


@pytest.mark.parametrize('kind,store', [('fuseunet', True), ('UNet', True), ('fuseunet', False)])
def test_bf16_network_vs_bf16_oracle(dev, kind, store):
    """precision='bf16' against the oracle whose 3x3 convolutions use bf16-rounded operands (oracle/bf16.py) for the
    same layers: logits, loss and every parameter gradient.  A bf16 rounding point is a discontinuity like a ReLU
    mask: an fp32-noise difference before the rounding moves the value by a whole bf16 ulp (2^-8 relative).  With the
    conv output z stored as bf16 (`store`, the default) ~3e-4 of all z values land on the other side of a rounding
    boundary in any two implementations that sum in a different order, and this random-init, 2-image, 64x64 network
    amplifies perturbations (the full bf16 rounding moves its logits by 10 %).  Measured here: logits 1.8-3.2e-2 of
    their scale, loss 7e-5, worst parameter gradient 3.5e-2, 0.3 % ReLU-mask flips; bounds 6e-2 / 2e-3 / 8e-2 (fp32-stored
    z: 1e-2 / 5e-3 / 5e-2).  The kernels themselves are held to 3e-5 / bit-exactness above -- that is the parity
    evidence; this test guards the wiring (which layers run where, storage types, gradient flow)."""
    from oracle import bf16 as OB
    LOGIT_TOL, LOSS_TOL, GRAD_TOL = (6e-2, 2e-3, 8e-2) if store else (1.5e-2, 5e-3, 5e-2)   # (measured 0.8e-2 .. 1.02e-2 across summation orders)
    OB.STORE_Z_BF16[0] = OB.STORE_A_BF16[0] = OB.STORE_G_BF16[0] = store          # (the oracle's own emulation switches)
    try:
        _network_vs_oracle(dev, kind, LOGIT_TOL, LOSS_TOL, GRAD_TOL, store)
    finally:
        OB.STORE_Z_BF16[0] = OB.STORE_A_BF16[0] = OB.STORE_G_BF16[0] = True


def _network_vs_oracle(dev, kind, LOGIT_TOL, LOSS_TOL, GRAD_TOL, store=True):
    import oracle
    from aide_amd import utils as U
    from aide_amd.engine import BF16
    net, ref = _pair(dev, kind, store)
    g = torch.Generator().manual_seed(1234)
    n, s = 2, 64
    xs = [torch.randn(n, 3, s, s, generator=g) for _ in range(2 if kind == 'fuseunet' else 1)]
    t = (torch.rand(n, s, s, generator=g) > 0.7).long()
    w = torch.tensor([1.0, 1.0])
    ref.train(); net.train()
    out = net(*[x.to(dev) for x in xs])
    loss = U.CEMDiceLoss(cediceweight=w, ceclassweight=w, diceclassweight=w)(out, t.to(dev))
    loss.backward()
    plan = list(net.engine.plans.values())[0]
    # the oracle's backward runs on OUR ReLU masks / pooling winners (tests/test_gpu_models.py: a mask element that
    # flips because the two forwards differ in the last digits is a property of the arithmetic, not of either side)
    from test_gpu_models import forced_relu_masks
    with forced_relu_masks(net, ref, plan) as fm:
        out_r = ref(*xs)
        loss_r = oracle.CEMDiceLoss(cediceweight=w, ceclassweight=w, diceclassweight=w)(out_r, t)
        loss_r.backward()
    # (z is stored as bf16: an fp32-noise difference in an accumulator moves z by a whole bf16 ulp, so a BatchNorm output
    # near zero changes sign far more often than between two fp32 implementations -- 0.3 % of the mask elements here)
    assert sum(fm.flips.values()) <= 1e-2 * fm.total, 'implausibly many ReLU mask flips: %d of %d' % (
        sum(fm.flips.values()), fm.total)
    modes = [(st['wino_f'], st['wino_d'], st['wino_w']) for st in plan.steps if st['kind'] == 'conv']
    assert sum(m[0] == BF16 for m in modes) >= 8 and sum(m[2] == BF16 for m in modes) >= 6, modes
    print('bf16 network parity: logits %.3e loss %.3e flips %d/%d' % (
        _rel(out, out_r), abs(loss.item() - loss_r.item()) / abs(loss_r.item()), sum(fm.flips.values()), fm.total))
    assert _rel(out, out_r) < LOGIT_TOL, 'logits %g' % _rel(out, out_r)
    assert abs(loss.item() - loss_r.item()) < LOSS_TOL * abs(loss_r.item())
    worst = 0.0
    for (name, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        if name.endswith('conv1.bias') or name.endswith('conv2.bias') or '.bilinear_up.' in name and name.endswith('.1.bias'):
            continue                                   # biases feeding a BatchNorm: zero true gradient (HISTORY §5)
        scale = q.grad.abs().max().item()
        if scale < 1e-7:
            continue
        worst = max(worst, (p.grad.cpu() - q.grad).abs().max().item() / scale)
    print('worst parameter-gradient error %.3e' % worst)
    assert worst < GRAD_TOL, 'worst parameter-gradient error %g' % worst


def test_bf16_mode_close_to_fp32_mode(dev):
    """The bf16 mode is a bounded perturbation of the fp32 mode (this small random-init network amplifies the 2^-9
    operand rounding to ~10 % of the logit scale: bound 0.3) and training still reduces the loss."""
    from aide_amd import utils as U
    from aide_amd.optim import Adam
    from aide_amd.models_twomodalinputs import fuseunet
    g = torch.Generator().manual_seed(7)
    x1 = torch.randn(2, 3, 64, 64, generator=g).to(dev)
    x2 = torch.randn(2, 3, 64, 64, generator=g).to(dev)
    t = (torch.rand(2, 64, 64, generator=g) > 0.7).long().to(dev)
    w = torch.tensor([1.0, 1.0])
    crit = U.CEMDiceLoss(cediceweight=w, ceclassweight=w, diceclassweight=w)
    outs = {}
    for prec in ('fp32', 'bf16'):
        torch.manual_seed(2)
        net = fuseunet(2).to(dev)
        net.engine.precision = prec
        assert net.engine.precision == prec
        net.train()
        outs[prec] = net(x1, x2).detach().clone()
        if prec == 'bf16':
            opt = Adam(net.parameters(), lr=1e-3, amsgrad=True)
            losses = []
            for _ in range(6):
                opt.zero_grad()
                loss = crit(net(x1, x2), t)
                loss.backward()
                opt.step()
                losses.append(loss.item())
            assert losses[-1] < losses[0], losses
    assert _rel(outs['bf16'], outs['fp32']) < 0.3
    with pytest.raises(ValueError):
        net.engine.precision = 'fp16'


def test_bf16_step_is_bit_reproducible(dev):
    """Two identical training steps of the bf16 mode at 256x256 (all three conv tile variants, the LDS epilogue, the 8-wave
    kernels, split-K and slab reductions, bf16 read-add-round accumulation) give bit-identical logits, loss and parameter
    gradients: no atomics, no races, fixed summation orders."""
    from aide_amd import utils as U
    from aide_amd.models_twomodalinputs import fuseunet
    g = torch.Generator().manual_seed(11)
    x1 = torch.randn(2, 3, 256, 256, generator=g).to(dev)
    x2 = torch.randn(2, 3, 256, 256, generator=g).to(dev)
    t = (torch.rand(2, 256, 256, generator=g) > 0.7).long().to(dev)
    w = torch.tensor([1.0, 1.0])
    crit = U.CEMDiceLoss(cediceweight=w, ceclassweight=w, diceclassweight=w)
    runs = []
    for _ in range(2):
        torch.manual_seed(2)
        net = fuseunet(2).to(dev)
        net.engine.precision = 'bf16'
        net.train()
        out = net(x1, x2)
        loss = crit(out, t)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((out.detach().clone(), loss.detach().clone(), [p.grad.clone() for p in net.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for a, b in zip(runs[0][2], runs[1][2]):
        assert torch.equal(a, b)
    assert torch.isfinite(runs[0][1])
