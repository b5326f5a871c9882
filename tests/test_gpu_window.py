"""-m gpu: sliding-window inference on the device (aide_amd/csrc/window.hip, aide_amd/window.py).  `aide_window_stack` is the
clamped window stack of window_cases byte for byte; `aide_window_blend` meets the float64 statement on the six cases
(probabilities within PROB_TOL, labels equal at every pixel: the cases' float64 top-two gaps exceed MIN_GAP) and repeats its
bytes from call to call; with uniform weights and overlap along one axis a stacked and blended map gives the bits of
`ensemble_vote([L], (0,))` and `label_map(L)` (p + p and the division by 2 are exact), which fails on a wrong window offset,
clamp, raster order or tile edge; refused arguments launch nothing; and `predict_labels(..., window=...)` and `predict_case`
equal the chain composed from these parts.  With probabilities in, the device bytes are `window_blend_host`'s (no product is
contracted into a sum); the device soft-max is not asserted byte-equal to it: the exponentials of the two libraries differ."""
import ctypes

import pytest
import torch

import window_cases as wc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('idx', range(len(wc.CASES)), ids=wc.IDS)
def test_window_stack_is_the_definition(dev, idx):
    from aide_amd.inference import window_stack
    N, C, H, W, window, stride = wc.CASES[idx][:6]
    x = torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(50 + idx))
    want = wc.stack(x, window, stride)
    got = window_stack(x.to(dev), window, stride)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got.cpu(), want)
    # a non-contiguous input is read through a contiguous copy
    xt = x.transpose(0, 1)
    assert torch.equal(window_stack(xt.to(dev), window, stride).cpu(), wc.stack(xt, window, stride))


@pytest.mark.parametrize('idx', range(len(wc.CASES)), ids=wc.IDS)
def test_blend_against_float64(dev, idx):
    from aide_amd.inference import window_blend
    N, C, H, W, window, stride, weights = wc.CASES[idx][:7]
    z = wc.case_logits(idx)
    want_l, want_p, gap = wc.case_reference(idx)
    assert gap > wc.MIN_GAP
    zd = z.to(dev)
    labels, probs = window_blend(zd, (H, W), window, stride, weights, probs=True)
    assert labels.is_cuda and labels.dtype == torch.int64 and probs.dtype == torch.float32
    assert tuple(labels.shape) == (N, H, W) and tuple(probs.shape) == (N, C, H, W)
    err = (probs.cpu().double() - want_p).abs().max().item()
    print('max |p - p64| = %.3e (gap %.3e)' % (err, gap))
    assert err <= wc.PROB_TOL
    assert torch.equal(labels.cpu(), want_l)
    l2, p2 = window_blend(zd, (H, W), window, stride, weights, probs=True)           # the same bytes from call to call
    assert torch.equal(l2, labels) and torch.equal(p2, probs)
    assert torch.equal(window_blend(zd, (H, W), window, stride, weights), labels)    # without the probabilities
    l4, p4 = window_blend(zd.reshape((-1,) + tuple(zd.shape[2:])), (H, W), window, stride, weights, probs=True)   # [B*N,C,wh,ww]
    assert torch.equal(l4, labels) and torch.equal(p4, probs)


@pytest.mark.parametrize('idx', range(len(wc.CASES)), ids=wc.IDS)
def test_blend_of_probabilities_is_the_host_statement(dev, idx):
    """With probabilities in, no exponential is involved: the blend is products, sums and one division, each rounded to fp32 on
    its own, so the device bytes are `window_blend_host`'s.  Gaussian weights on every case (coverage up to 9): a product
    contracted into the sum that consumes it, or a `den` that adds an unrounded weight, changes last bits."""
    from aide_amd.inference import window_blend, window_blend_host
    N, C, H, W, window, stride = wc.CASES[idx][:6]
    p = torch.softmax(wc.case_logits(idx), 2)
    for weights, sigma in (('gaussian', 0.125), ('gaussian', 0.3), ('uniform', 0.125)):
        want_l, want_p = window_blend_host(p, (H, W), window, stride, weights, sigma, logits=False, probs=True)
        labels, probs = window_blend(p.to(dev), (H, W), window, stride, weights, sigma, logits=False, probs=True)
        diff = int((probs.cpu() != want_p).sum())
        print('%s %.3f: %d of %d probabilities differ from the host statement' % (weights, sigma, diff, want_p.numel()))
        assert diff == 0 and torch.equal(labels.cpu(), want_l)


@pytest.mark.parametrize('idx', range(len(wc.EXACT)), ids=['40x32', '32x48', '9x40-padded', '48x48-32x16'])
def test_blend_geometry_exact(dev, idx):
    from aide_amd.inference import window_stack, window_blend, ensemble_vote, label_map
    H, W, window, stride = wc.EXACT[idx]
    Ld = wc.exact_logits(idx).to(dev)
    one_l, one_p = ensemble_vote([Ld], (0,), probs=True)
    assert torch.equal(one_l, label_map(Ld))
    labels, probs = window_blend(window_stack(Ld, window, stride), (H, W), window, stride, 'uniform', probs=True)
    assert torch.equal(probs, one_p), '%d pixels differ' % int((probs != one_p).any(1).sum())
    assert torch.equal(labels, one_l)
    l2, p2 = window_blend(window_stack(one_p, window, stride), (H, W), window, stride, 'uniform', logits=False, probs=True)
    assert torch.equal(p2, one_p) and torch.equal(l2, one_l)


def test_bad_arguments_launch_nothing(dev):
    from aide_amd._lib import lib
    from aide_amd.ops import ptr, stream_ptr
    from aide_amd.inference import window_blend, window_stack
    z = torch.zeros(6, 1, 2, 16, 16, device=dev)                    # the grid of a 24 x 40 image: 2 x 3 windows
    good = dict(image_size=(24, 40), window=16, stride=(8, 12))
    assert window_blend(z, **good).eq(0).all()
    for values, change in ((z[0, 0], {}), (z.double(), {}), (torch.zeros(6, 1, 1, 16, 16, device=dev), {}),
                           (torch.zeros(6, 1, 9, 16, 16, device=dev), {}), (z[:5], {}), (z.reshape(6, 2, 16, 16)[:4], {}),
                           (z, dict(window=(16, 32))), (z, dict(stride=(8, 17))), (z, dict(weights='hann')),
                           (z, dict(image_size=(16 + 32 * 4, 16), stride=4))):
        with pytest.raises(ValueError):
            window_blend(values, **dict(good, **change))
    x = torch.zeros(1, 3, 24, 40, device=dev)
    for bad, window, stride in ((x[0], 16, 8), (x.double(), 16, 8), (x, 16, 17), (x, 0, None), (x, 1, 1)):   # the last: 40 starts
        with pytest.raises(ValueError):
            window_stack(bad, window, stride)
    # the C ABI itself, with real device memory: refused, and the outputs keep their bytes
    H, W, wh = 40, 24, 16
    src = torch.zeros(4 * 2, 1, 2, wh, wh, device=dev)
    xin = torch.zeros(1, 2, H, W, device=dev)
    g = torch.ones(wh, device=dev)
    labels = torch.full((1, H, W), -7, device=dev, dtype=torch.int64)
    probs = torch.full((1, 2, H, W), -7.0, device=dev)
    y = torch.full((4 * 2, 1, 2, wh, wh), -7.0, device=dev)

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def blend(sy=(0, 8, 16, 24), sx=(0, 8), c=2):
        return lib.aide_window_blend(ptr(src), 1, 2 * wh * wh, 1, c, H, W, wh, wh, ints(*sy), len(sy), ints(*sx), len(sx), ptr(g), ptr(g),
                                     ptr(labels), ptr(probs), 2 * H * W, stream_ptr())

    def stack(sy=(0, 8, 16, 24), sx=(0, 8)):
        return lib.aide_window_stack(ptr(xin), 2 * H * W, ptr(y), 2 * wh * wh, 1, 2, H, W, wh, wh, ints(*sy), len(sy), ints(*sx), len(sx),
                                     stream_ptr())

    for call in (blend, stack):
        assert call(sy=(0, 4, 24)) == -1                              # a gap between starts
        assert call(sy=(8, 16, 24)) == -1                             # the first start is not 0
        assert call(sy=(0, 8, 16)) == -1                              # the last window short of the border
        assert call(sy=(0, 16, 8, 24)) == -1                          # decreasing starts
        assert call(sx=(0, 9)) == -1                                  # a start beyond W - ww
    assert blend(c=9) == -1 and blend(c=1) == -1
    torch.cuda.synchronize()
    assert labels.eq(-7).all() and probs.eq(-7.0).all() and y.eq(-7.0).all()
    assert blend() == 0 and stack() == 0                              # the same calls with a valid grid run
    torch.cuda.synchronize()
    assert labels.eq(0).all() and probs.eq(0.5).all() and y.eq(0.0).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _net(dev, kind, classes, seed=5):
    from aide_amd.models_singlemodalinput import UNet
    from aide_amd.models_twomodalinputs import fuseunet
    torch.manual_seed(seed)
    net = (fuseunet(classes) if kind == 'fuseunet' else UNet(classes)).to(dev)
    net.eval()
    return net


def _inputs(dev, kind, s, h, w, seed=21):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(s, 3, h, w, generator=g).to(dev) for _ in range(2 if kind == 'fuseunet' else 1))


def _composed(net, xs, window, stride, views, chunk, group, probs=False):
    """window_stack -> net (-> ensemble_vote(probs=True) per window image) -> window_blend, `group` slices at a time and
    `chunk` window images per forward"""
    from aide_amd.inference import window_stack, window_blend, ensemble_logits, ensemble_vote, view_codes
    h, w = xs[0].shape[-2:]
    out = []
    with torch.no_grad():
        for i in range(0, xs[0].shape[0], group):
            stacks = [window_stack(x[i:i + group], window, stride) for x in xs]
            b, g = stacks[0].shape[:2]
            stacks = [s.reshape((b * g,) + tuple(s.shape[2:])) for s in stacks]
            maps = []
            for j in range(0, b * g, chunk):
                part = [s[j:j + chunk] for s in stacks]
                if views is None:
                    maps.append(net(*part))
                else:
                    codes = view_codes(views, *part[0].shape[-2:])
                    maps.append(ensemble_vote(list(ensemble_logits(net, *part, views=views)), codes, probs=True)[1])
            out.append(window_blend(torch.cat(maps), (h, w), window, stride, logits=views is None, probs=probs))
    if probs:
        return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])
    return torch.cat(out)


@pytest.mark.parametrize('kind,classes,hw,window,stride,views',
                         [('UNet', 2, (48, 80), 32, 16, None), ('fuseunet', 2, (40, 40), 32, None, None),
                          ('UNet', 3, (48, 80), 32, 16, 'flip2')], ids=['unet-48x80', 'fuseunet-40x40', 'unet3-flip2'])
def test_predict_labels_equals_its_parts(dev, kind, classes, hw, window, stride, views):
    from aide_amd.inference import predict_labels, predict_case, window_grid, keep_largest_connected_components
    net = _net(dev, kind, classes)
    xs = _inputs(dev, kind, 2, *hw)
    sy, sx = window_grid(hw[0], hw[1], window, stride)
    B, V = len(sy) * len(sx), 1 if views is None else 2
    kw = dict(window=window, stride=stride, views=views)
    # one forward batch
    want, want_p = _composed(net, xs, window, stride, views, chunk=B * 2, group=2, probs=True)
    got = predict_labels(net, *xs, batch_size=B * 2 * V, **kw)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2,) + hw and torch.equal(got, want)
    # a small batch_size: groups of max(1, batch_size // (B * V)) slices, chunks of max(1, batch_size // V) window images
    bs = 4
    small = predict_labels(net, *xs, batch_size=bs, **kw)
    assert torch.equal(small, _composed(net, xs, window, stride, views, chunk=max(1, bs // V), group=max(1, bs // (B * V))))
    # predict_case: the filtered volume of the blended labels, and the blended probabilities on request
    vol = predict_case(net, *xs, keep_largest=True, numpy=False, batch_size=B * 2 * V, **kw)
    assert vol.dtype == torch.uint8 and torch.equal(vol, keep_largest_connected_components(want.permute(1, 2, 0)))
    vol2, pr = predict_case(net, *xs, probs=True, numpy=False, batch_size=B * 2 * V, **kw)
    assert torch.equal(vol2, want.permute(1, 2, 0)) and torch.equal(pr, want_p) and tuple(pr.shape) == (2, classes) + hw
    assert predict_case(net, *xs, batch_size=B * 2 * V, **kw).shape == hw + (2,)


def test_single_window_is_the_plain_path_and_sizes(dev):
    from aide_amd.inference import predict_labels
    net = _net(dev, 'UNet', 2)
    (x,) = _inputs(dev, 'UNet', 2, 32, 48)
    plain = predict_labels(net, x)                                    # today's path, unchanged
    assert plain.dtype == torch.int64 and tuple(plain.shape) == (2, 32, 48)
    # one window of weight 1 over the whole image
    assert torch.equal(predict_labels(net, x, window=(32, 48), window_weights='uniform'), plain)
    (odd,) = _inputs(dev, 'UNet', 2, 40, 56, seed=22)                 # 40 is no multiple of 16: only windows predict it
    got = predict_labels(net, odd, window=32)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, 40, 56) and int(got.min()) >= 0 and int(got.max()) <= 1
    with pytest.raises(ValueError):
        predict_labels(net, odd, window=24)                           # not a multiple of 16
    with pytest.raises(ValueError):
        predict_labels(net, odd, window=(32, 16), views='d4')         # a quarter turn of a non-square window
    with pytest.raises(TypeError):
        predict_labels(net, odd, stride=8)
    net.train()
    with pytest.raises(RuntimeError):
        predict_labels(net, odd, window=32)
    net.eval()
