"""Host side of sliding-window inference (aide_amd/window.py): the grid against its rules, the CPU window stack against the
case module's, `window_blend_host` (the statement the device kernel is held to) against the float64 statement on the six
cases of window_cases, the exactness property the device test relies on, and the grouping and chunking of
`predict_labels(..., window=...)` through a stub network on CPU tensors.  No GPU."""
import subprocess

import pytest
import torch

import window_cases as wc


@pytest.mark.parametrize('size,win,stride', [(40, 16, 8), (37, 16, 16), (16, 16, 8), (9, 16, 8), (70, 32, 12), (50, 16, 6),
                                             (512, 256, 128), (17, 16, 1), (33, 32, 32), (100, 7, 7), (47, 16, 16)])
def test_grid_rules(size, win, stride):
    from aide_amd.inference import window_grid
    sy, sx = window_grid(size, 23, (win, 16), (stride, 8))
    assert isinstance(sy, tuple) and all(isinstance(v, int) for v in sy)
    assert list(sy) == wc.starts(size, win, stride) and list(sx) == wc.starts(23, 16, 8)
    assert sy[0] == 0 and sy[-1] == max(0, size - win)               # the last window ends at the border
    assert all(0 < b - a <= stride for a, b in zip(sy, sy[1:]))
    covered = torch.zeros(size, dtype=torch.bool)
    for s in sy:
        covered[s:s + win] = True
    assert covered.all()
    if size <= win:
        assert sy == (0,)


def test_grid_defaults_and_errors():
    from aide_amd.inference import window_grid, window_weights
    assert window_grid(512, 384, 256) == ((0, 128, 256), (0, 128))   # stride None: half the window
    assert window_grid(40, 56, (16, 32), 8) == (tuple(wc.starts(40, 16, 8)), tuple(wc.starts(56, 32, 8)))
    assert window_grid(8, 8, 16) == ((0,), (0,))
    assert len(window_grid(16 + 31 * 4, 16, 16, 4)[0]) == 32          # 32 starts are allowed
    for args in ((40, 40, 0), (40, 40, -16), (40, 40, 16, 0), (40, 40, 16, 17), (40, 40, (16, 16), (8, 17)), (0, 40, 16),
                 (40, 40, (16, 16, 16)), (40, 40, 16.0), (16 + 32 * 4, 16, 16, 4), (16, 600, 16, (8, 1))):
        with pytest.raises(ValueError):
            window_grid(*args)
    gh, gw = window_weights((16, 32))
    assert gh.dtype == torch.float32 and tuple(gh.shape) == (16,) and tuple(gw.shape) == (32,) and not gh.is_cuda
    assert torch.equal(gh, wc.axis_weights(16, 'gaussian')) and torch.equal(gw, wc.axis_weights(32, 'gaussian'))
    assert torch.equal(gh, gh.flip(0)) and float(gh[0] * gh[0]) > 1.1754944e-38          # symmetric; the corner is a normal fp32
    assert all(torch.equal(g, torch.ones(n)) for g, n in zip(window_weights((8, 4), 'uniform'), (8, 4)))
    with pytest.raises(ValueError):
        window_weights(16, 'hann')
    with pytest.raises(ValueError):
        window_weights(16, 'gaussian', 0.0)
    # a corner weight that is no normal fp32 number would leave 0 / 0 in the corners of the image: refused, the least that works is not
    for win in (16, (256, 256), (16, 32)):
        with pytest.raises(ValueError):
            window_weights(win, 'gaussian', 0.05)
        gh, gw = window_weights(win, 'gaussian', 0.06)
        assert float(gh[0] * gw[0]) >= 1.1754944e-38 and float(gh[-1] * gw[-1]) >= 1.1754944e-38
    with pytest.raises(ValueError):
        window_weights(16, 'gaussian', float('nan'))


@pytest.mark.parametrize('idx', range(len(wc.CASES)), ids=wc.IDS)
def test_stack_host_is_the_definition(idx):
    from aide_amd.inference import window_stack
    N, C, H, W, window, stride = wc.CASES[idx][:6]
    x = torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(idx))
    got = window_stack(x, window, stride)
    want = wc.stack(x, window, stride)
    assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got, want)
    assert got.shape[0] == wc.case_logits(idx).shape[0]
    for bad in (x[0], x.double()):
        with pytest.raises(ValueError):
            window_stack(bad, window, stride)


@pytest.mark.parametrize('idx', range(len(wc.CASES)), ids=wc.IDS)
def test_blend_host_against_float64(idx):
    from aide_amd.inference import window_blend, window_blend_host
    N, C, H, W, window, stride, weights = wc.CASES[idx][:7]
    z = wc.case_logits(idx)
    want_l, want_p, gap = wc.case_reference(idx)
    print('smallest float64 top-two gap %.3e' % gap)
    assert gap > wc.MIN_GAP
    labels, probs = window_blend_host(z, (H, W), window, stride, weights, probs=True)
    err = (probs.double() - want_p).abs().max().item()
    print('max |p - p64| = %.3e' % err)
    assert labels.dtype == torch.int64 and probs.dtype == torch.float32 and tuple(probs.shape) == (N, C, H, W)
    assert err <= wc.PROB_TOL
    assert torch.equal(labels, want_l)
    assert torch.equal(window_blend_host(z, (H, W), window, stride, weights), labels)
    l2, p2 = window_blend(z.reshape((-1,) + tuple(z.shape[2:])), (H, W), window, stride, weights, probs=True)   # CPU: the host statement
    assert torch.equal(l2, labels) and torch.equal(p2, probs)
    # probabilities in: the same blend of the fp32 soft-max maps
    l3, p3 = window_blend_host(torch.softmax(z, 2), (H, W), window, stride, weights, logits=False, probs=True)
    assert (p3.double() - want_p).abs().max().item() <= wc.PROB_TOL and torch.equal(l3, want_l)


@pytest.mark.parametrize('idx', range(len(wc.EXACT)))
def test_blend_host_geometry_exact(idx):
    """coverage 1 or 2 with uniform weights: p + p and the division by 2 are exact, so a stacked map blends to its own bits"""
    from aide_amd.inference import window_stack, window_blend_host, ensemble_vote_host
    H, W, window, stride = wc.EXACT[idx]
    L = wc.exact_logits(idx)
    one_l, one_p = ensemble_vote_host([L], (0,), probs=True)
    labels, probs = window_blend_host(window_stack(L, window, stride), (H, W), window, stride, 'uniform', probs=True)
    assert torch.equal(probs, one_p) and torch.equal(labels, one_l)
    l2, p2 = window_blend_host(window_stack(one_p, window, stride), (H, W), window, stride, 'uniform', logits=False, probs=True)
    assert torch.equal(p2, one_p) and torch.equal(l2, one_l)


def test_blend_bad_arguments():
    from aide_amd.inference import window_blend
    z = torch.zeros(6, 1, 2, 16, 16)                               # the grid of a 24 x 40 image: 2 x 3 windows
    assert window_blend(z, (24, 40), 16, (8, 12)).eq(0).all()
    for values, size, window, stride, weights in (
            (z[0, 0], (24, 40), 16, (8, 12), 'uniform'), (z.double(), (24, 40), 16, (8, 12), 'uniform'),
            (torch.zeros(6, 1, 1, 16, 16), (24, 40), 16, (8, 12), 'uniform'), (torch.zeros(6, 1, 9, 16, 16), (24, 40), 16, (8, 12), 'uniform'),
            (z[:5], (24, 40), 16, (8, 12), 'uniform'), (z.reshape(6, 2, 16, 16)[:4], (24, 40), 16, (8, 12), 'uniform'),
            (z, (24, 40), (16, 32), (8, 12), 'uniform'), (z, (24, 40), 16, (8, 17), 'uniform'), (z, (24, 40), 16, (8, 12), 'hann'),
            (z, (16 + 32 * 4, 16), 16, 4, 'uniform')):
        with pytest.raises(ValueError):
            window_blend(values, size, window, stride, weights)


class _Stub(torch.nn.Module):
    """logits that depend on the pixel and on where it lies in the window: class c gets w_c * x + b_c * ramp.  Records the
    batch shapes it is called with."""

    def __init__(self, classes, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = torch.nn.Parameter(torch.randn(classes, generator=g))
        self.b = torch.nn.Parameter(torch.randn(classes, generator=g))
        self.calls = []

    def forward(self, *xs):
        self.calls.append(tuple(tuple(x.shape) for x in xs))
        x = sum(t.sum(1, keepdim=True) for t in xs)
        ramp = torch.linspace(-1, 1, x.shape[-1]).view(1, 1, 1, -1) + torch.linspace(0, 0.5, x.shape[-2]).view(1, 1, -1, 1)
        return x * self.w.view(1, -1, 1, 1) + ramp * self.b.view(1, -1, 1, 1)


def test_predict_labels_window_groups_and_chunks():
    from aide_amd.inference import predict_labels, predict_case, window_stack, window_blend_host, ensemble_vote_host, \
        view_apply_host
    g = torch.Generator().manual_seed(13)
    a, b = torch.randn(5, 3, 40, 56, generator=g), torch.randn(5, 3, 40, 56, generator=g)
    net = _Stub(3, 1).eval()
    B = 2 * 3                                                     # window 32, stride 16 on 40 x 56
    with torch.no_grad():
        z = net(window_stack(a, 32, 16).reshape(-1, 3, 32, 32), window_stack(b, 32, 16).reshape(-1, 3, 32, 32))
    want_l, want_p = window_blend_host(z, (40, 56), 32, 16, probs=True)
    # groups of max(1, batch_size // B) slices, a group's B * g window images in chunks of at most batch_size
    for bs, shapes in ((64, [30]), (12, [12, 12, 6]), (16, [12, 12, 6]), (4, [4, 2] * 5), (1, [1] * 30)):
        net.calls = []
        got = predict_labels(net, a, b, window=32, stride=16, batch_size=bs)
        assert [c[0][0] for c in net.calls] == shapes, (bs, net.calls)
        assert all(c == ((c[0][0], 3, 32, 32),) * 2 for c in net.calls)
        assert got.dtype == torch.int64 and torch.equal(got, want_l), bs
    vol, pr = predict_case(net, a, b, window=32, stride=16, probs=True, numpy=False, batch_size=64)
    assert torch.equal(vol, want_l.permute(1, 2, 0)) and torch.equal(pr, want_p)
    assert predict_case(net, a, b, window=32, stride=16).shape == (40, 56, 5)
    # with views: per window image the vote's mean soft-max, blended as probabilities; g = max(1, batch_size // (B * V))
    with torch.no_grad():
        stacks = [window_stack(t, 32, 16).reshape(-1, 3, 32, 32) for t in (a, b)]
        members = [net(*[view_apply_host(s, v) for s in stacks]) for v in (0, 4)]
    mean = ensemble_vote_host(members, (0, 4), probs=True)[1]
    voted_l, voted_p = window_blend_host(mean, (40, 56), 32, 16, logits=False, probs=True)
    for bs, shapes in ((64, [60]), (24, [24, 24, 12]), (6, [6, 6] * 5)):
        net.calls = []
        got = predict_labels(net, a, b, window=32, stride=16, views='flip2', batch_size=bs)
        assert [c[0][0] for c in net.calls] == shapes, (bs, net.calls)
        assert torch.equal(got, voted_l), bs
    vol, pr = predict_case(net, a, b, window=32, stride=16, views='flip2', probs=True, numpy=False)
    assert torch.equal(vol, voted_l.permute(1, 2, 0)) and torch.equal(pr, voted_p)
    # one window of weight 1 over the whole image: the plain arg-max of the soft-max
    with torch.no_grad():
        plain = torch.softmax(net(a[..., :32, :48], b[..., :32, :48]), 1).argmax(1)
    assert torch.equal(predict_labels(net, a[..., :32, :48], b[..., :32, :48], window=(32, 48), window_weights='uniform'), plain)


def test_predict_labels_window_errors():
    from aide_amd.inference import predict_labels, predict_case
    x = torch.zeros(2, 3, 40, 40)
    net = _Stub(2, 1).eval()
    for kw in (dict(stride=8), dict(window_weights='uniform'), dict(sigma_scale=0.25), dict(stride=8, views='flip2')):
        with pytest.raises(TypeError):
            predict_labels(net, x, **kw)
        with pytest.raises(TypeError):
            predict_case(net, x, probs=True, **kw)
    for kw in (dict(window=24), dict(window=(32, 40)), dict(window=(32, 16), views='d4'), dict(window=32, stride=33),
               dict(window=32, window_weights='hann'), dict(window=32, views=(0,) * 17)):
        with pytest.raises(ValueError):
            predict_labels(net, x, **kw)
    with pytest.raises(ValueError):
        predict_labels(net, x, window=32, sigma_scale=0.01)        # the corner weights underflow
    for inputs in ((x, x[..., :32]), (x, x[:1]), (x.double(),), (x[0],)):     # modalities that differ, dtype, rank
        with pytest.raises(ValueError, match='predict_windows'):
            predict_labels(net, *inputs, window=32)
    assert net.calls == []                                         # refused before any forward
    with pytest.raises(ValueError):
        predict_labels(net, torch.zeros(1, 3, 16 + 32 * 4, 16), window=16, stride=4)     # 33 starts
    with pytest.raises(TypeError):
        predict_labels(net, x, window=32, overlap=0.5)
    net.train()
    with pytest.raises(RuntimeError):
        predict_labels(net, x, window=32)


@pytest.fixture(scope='module')
def built():
    from aide_amd.build import build
    return build(verbose=False)


def test_header_declares_and_library_exports(built):
    from aide_amd._lib import lib, parse_header
    protos = parse_header()
    out = subprocess.run(['nm', '-D', '--defined-only', built], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name, nargs in (('aide_window_stack', 15), ('aide_window_blend', 19)):
        assert name in protos and name in lib.protos and name in exported, name
        assert len(protos[name][1]) == nargs


def test_abi_rejects_bad_arguments_before_any_launch(built):
    """AIDE_ERR_ARG (-1) from both entry points with no device memory behind the pointers: nothing can have been launched"""
    import ctypes
    from aide_amd._lib import lib
    fake = ctypes.c_void_p(4096)

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def table(v, count):
        return (None if v is None else ints(*v)), (len(v or ()) if count is None else count)

    def stack(x=fake, y=fake, N=1, C=3, H=40, W=16, wh=16, ww=16, sy=(0, 8, 16, 24), sx=(0,), ny=None, nx=None):
        return lib.aide_window_stack(x, C * H * W, y, C * wh * ww, N, C, H, W, wh, ww, *table(sy, ny), *table(sx, nx), None)

    def blend(src=fake, N=1, C=2, H=40, W=16, wh=16, ww=16, sy=(0, 8, 16, 24), sx=(0,), gh=fake, gw=fake, labels=fake, ny=None,
              nx=None):
        return lib.aide_window_blend(src, 1, C * wh * ww, N, C, H, W, wh, ww, *table(sy, ny), *table(sx, nx), gh, gw, labels, None,
                                     C * H * W, None)

    for call in (stack, blend):
        assert call(sy=None, ny=1) == -1 and call(sx=None, nx=1) == -1
        assert call(sy=(0, 8, 16, 25)) == -1                          # a start beyond size - win
        assert call(sy=(0, 16, 8, 24)) == -1 and call(sy=(0, 8, 8, 24)) == -1      # not increasing
        assert call(sy=(8, 16, 24)) == -1                             # the first start is not 0
        assert call(sy=(0, 8, 16)) == -1                              # the last window short of the border
        assert call(sy=(0, 4, 24)) == -1                              # a gap above the window
        assert call(sy=(-1, 8, 16, 24)) == -1
        assert call(sy=tuple(range(25)) + tuple(range(25, 33)), H=48) == -1        # 33 starts
        assert call(sy=(), ny=0) == -1
        assert call(sx=(0, 8), W=16) == -1                            # W <= ww: the only start is 0
        assert call(H=0, sy=(0,)) == -1 and call(wh=0) == -1 and call(N=0) == -1
        assert call(N=1 << 15, C=4, H=128, W=128, wh=128, ww=128, sy=(0,)) == -1   # 2^31 elements
    assert stack(x=None) == -1 and stack(y=None) == -1
    assert blend(src=None) == -1 and blend(gh=None) == -1 and blend(gw=None) == -1 and blend(labels=None) == -1
    assert blend(C=1) == -1 and blend(C=lib.aide_seg_max_classes() + 1) == -1
    # many windows of a small image: B * N * C * wh * ww reaches 2^31 although N * C * H * W does not
    many = tuple(range(0, 32))
    assert blend(N=1 << 10, C=8, H=16 + 31, W=16 + 31, sy=many, sx=many) == -1
