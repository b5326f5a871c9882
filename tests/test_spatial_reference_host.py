"""The references of tests/spatial_cases.py without a GPU: the float64 interpolation matrices against aten's own fp32
bilinear forward / backward, the float64 head against aten fp32, the written-out first-maximum pooling rule against aten's
max_pool2d on tie content, and the layout helper (strides, sentinel bookkeeping)."""
import pytest
import torch
import torch.nn.functional as F

import spatial_cases as S

UP_SIZES = [(1, 1), (3, 5), (7, 511), (3, 510), (16, 512), (20, 80), (18, 160), (48, 192)]


@pytest.mark.parametrize('size', UP_SIZES)
def test_interpolation_matrices_are_atens_bilinear(size):
    """y = Rh x Rw^T and dx = Rh^T dy Rw agree with aten's fp32 kernels to 1e-6 of the result scale (measured: <= 1e-7
    forward, <= 2e-7 backward); a float64 interpolate of the same input does not at the wide sizes, which is why it is not
    the reference"""
    h, w = size
    x, dy, _, y_ref, dx_ref = S.up_case(2, 3, h, w)
    xr = x.clone().requires_grad_(True)
    y = F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=True)
    y.backward(dy)
    S.assert_close(y, y_ref, 1e-6, 'forward %s' % (size,))
    S.assert_close(xr.grad, dx_ref, 1e-6, 'backward %s' % (size,))


@pytest.mark.parametrize('n', [1, 2, 3, 7, 80, 191, 335, 511, 512])
def test_interpolation_matrix_structure(n):
    r = S.interp_matrix(n)
    assert r.shape == (2 * n, n) and r.dtype == torch.float64
    assert float(r.min()) >= 0.0 and int((r != 0).sum(1).max()) <= 2
    assert float((r.sum(1) - 1.0).abs().max()) <= 2.0 ** -23            # l0 = float32(1 - l1): the pair sums to 1 within an ulp
    assert r[0, 0] == 1.0                                                 # align_corners: the first samples coincide
    assert abs(float(r[-1, -1]) - 1.0) <= 1e-4 * n                        # ... and the last, up to the rounding of scale * dst
    nz = (r != 0).float()
    first = nz.argmax(1)                                                  # i0 never decreases along the output
    assert bool((first[1:] >= first[:-1]).all())


def test_double_interpolate_is_not_the_operator():
    """the finding that fixed the reference: at W = 510 a float64 interpolate is off by more than the kernels' 5e-6"""
    x = S.up_case(2, 3, 3, 510)[0]
    y64 = F.interpolate(x.double(), scale_factor=2, mode='bilinear', align_corners=True)
    y32 = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True)
    assert S.rel_err(y32, y64) > 5e-6
    assert S.rel_err(y32, S.upsample_ref(x)) <= 1e-6


@pytest.mark.parametrize('k', [1, 2, 5, 8])
@pytest.mark.parametrize('c', [2, 7, 67])
def test_head_reference_against_aten_fp32(k, c):
    d = S.head_case(2, c, k, 8, 12)
    xr, wr, br = d['x'].clone().requires_grad_(True), d['w'].view(k, c, 1, 1).clone().requires_grad_(True), \
        d['b'].clone().requires_grad_(True)
    y = F.conv2d(xr, wr, br)
    y.backward(d['dy'])
    S.assert_close(y, d['y'], 2e-5, 'logits')
    S.assert_close(F.conv2d(d['x'], d['w'].view(k, c, 1, 1)), d['y_nobias'], 2e-5, 'logits without bias')
    S.assert_close(xr.grad, d['dx'], 2e-5, 'dx')
    S.assert_close(wr.grad.view(k, c), d['dw'], 2e-5, 'dw')
    S.assert_close(br.grad, d['db'], 2e-5, 'db')


def test_head_bn_reference_against_aten_fp32():
    d = S.head_case(2, 7, 5, 8, 12, bn=True)
    a = torch.relu(d['x'] * d['scale'].view(1, -1, 1, 1) + d['shift'].view(1, -1, 1, 1))
    clipped = float((a == 0).float().mean())
    assert 0.3 < clipped < 0.7                                            # about half of the activations
    wr = d['w'].view(5, 7, 1, 1).clone().requires_grad_(True)
    br = d['b'].clone().requires_grad_(True)
    y = F.conv2d(a, wr, br)
    y.backward(d['dy'])
    S.assert_close(y, d['y'], 2e-5, 'logits')
    S.assert_close(wr.grad.view(5, 7), d['dw'], 2e-5, 'dw')
    S.assert_close(br.grad, d['db'], 2e-5, 'db')


@pytest.mark.parametrize('hw', [(2, 2), (6, 10), (16, 24), (16, 18)])
def test_pool_tie_rule_is_atens(hw):
    """aten routes the gradient to the first maximum in row-major window order, on every tie class of pool_input"""
    x, dy, _, y, dx = S.pool_case(2, 5, hw[0], hw[1])
    m, d = S.pool_first_max(x, dy)
    assert torch.equal(m, y) and torch.equal(d, dx)
    assert float(dx[0, 3, 1::2].abs().max()) == 0.0 and float(dx[0, 3, :, 1::2].abs().max()) == 0.0     # -inf plane: element (0, 0)


def test_pool_input_holds_every_tie_class():
    x = S.pool_input(2, 5, 6, 8)
    win = torch.stack([x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]], -1)
    assert bool((win[:, 0] == win[:, 0, ..., :1]).all())                              # whole windows equal
    assert torch.equal(win[:, 1, ..., 0], win[:, 1, ..., 2]) and torch.equal(win[:, 1, ..., 1], win[:, 1, ..., 3])
    assert float(x[:, 2].max()) < 0.0
    assert bool(torch.isinf(x[0, 3]).all()) and float(x[0, 3].max()) < 0.0
    z = x[1, 3]
    assert float(z.abs().max()) == 0.0 and bool(torch.signbit(z).any()) and not bool(torch.signbit(z).all())
    top = win[:, 4].max(-1).values                                                    # the plain channel still ties often
    assert int(((win[:, 4] == top.unsqueeze(-1)).sum(-1) > 1).sum()) > 0


@pytest.mark.parametrize('kind', S.KINDS)
def test_layout_views(kind):
    shape = (2, 3, 4, 6)
    lay = S.Layout(kind, shape)
    val = torch.randn(shape)
    flat, v = lay.put(val, 'cpu')
    chw = 3 * 4 * 6
    assert v.shape == shape and v.stride()[1:] == (24, 6, 1)
    assert v.stride(0) == {'dense': chw, 'lo': 2 * chw, 'hi': 2 * chw, 'pad1': chw + 1, 'pad2': chw + 2, 'pad4': chw + 4}[kind]
    assert torch.equal(v, val) and lay.intact(flat)
    assert int((flat == S.SENT).sum()) == flat.numel() - val.numel()
    v.mul_(2.0)                                                           # writes inside the view are not "outside"
    assert lay.intact(flat)
    for i in (0, S.GUARD - 1, flat.numel() - 1, lay.offset + chw if kind != 'dense' else flat.numel() - S.GUARD):
        f = flat.clone()
        f[i] = 1.0                                                        # a guard element, the gap between two images
        assert not lay.intact(f)
    assert float(torch.tensor(S.SENT).bfloat16()) == S.SENT
