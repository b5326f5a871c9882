"""Host side of test-time augmentation (aide_amd/ensemble.py): the view algebra against its definition, `ensemble_vote_host`
(the statement the device kernel is held to) against a float64 statement on the five cases of ensemble_cases, and the member
order and chunking of `predict_labels(..., views=...)` through a stub network on CPU tensors.  No GPU."""
import ctypes
import subprocess

import pytest
import torch

import ensemble_cases as ec


def test_views_invert_and_sets():
    from aide_amd.inference import VIEW_SETS, view_apply_host, view_invert_host, view_codes
    assert VIEW_SETS == {'flip2': (0, 4), 'flip4': (0, 4, 2, 6), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}
    g = torch.Generator().manual_seed(7)
    for shape in ((2, 3, 5, 5), (4, 6, 6), (2, 3, 4, 7)):
        x = torch.randn(*shape, generator=g)
        seen = []
        for v in ec.valid_codes(*shape[-2:]):
            y = view_apply_host(x, v)
            assert torch.equal(y, ec.view_apply(x, v))
            assert torch.equal(view_invert_host(y, v), x) and torch.equal(view_apply_host(view_invert_host(x, v), v), x)
            assert tuple(y.shape[-2:]) == (tuple(shape[-2:])[::-1] if v & 1 else tuple(shape[-2:]))
            seen.append(y)
        # the views are distinct permutations of a generic image
        assert all(a.shape != b.shape or not torch.equal(a, b) for i, a in enumerate(seen) for b in seen[:i])
    assert view_codes('d4', 8, 8) == ec.D4 and view_codes('flip4', 3, 9) == (0, 4, 2, 6) and view_codes([4, 4, 0]) == (4, 4, 0)


@pytest.mark.parametrize('views,hw', [((), (4, 4)), ((8,), (4, 4)), ((-1,), (4, 4)), ((0, 1.0), (4, 4)), ('d8', (4, 4)),
                                      ('d4', (4, 6)), ((0, 3), (4, 6)), ((5,), (6, 4)), (3, (4, 4))])
def test_invalid_views_raise(views, hw):
    from aide_amd.inference import view_codes, view_stack, ensemble_vote
    with pytest.raises(ValueError):
        view_codes(views, *hw)
    x = torch.zeros(1, 2, *hw)
    with pytest.raises(ValueError):
        view_stack(x, views)
    if not isinstance(views, (str, int)):
        with pytest.raises(ValueError):
            ensemble_vote([x] * max(1, len(views)), views)


def test_invalid_single_codes_raise():
    from aide_amd.inference import view_apply_host, view_invert_host, ensemble_vote
    for fn in (view_apply_host, view_invert_host):
        for code, hw in ((8, (4, 4)), (-1, (4, 4)), (1, (4, 6)), (7, (6, 4))):
            with pytest.raises(ValueError):
                fn(torch.zeros(2, *hw), code)
    x = torch.zeros(1, 2, 4, 4)
    with pytest.raises(ValueError):
        ensemble_vote([x] * 17, (0,) * 17)                       # K > 16
    with pytest.raises(ValueError):
        ensemble_vote([x, x], (0,))                              # members and codes differ in number
    with pytest.raises(ValueError):
        ensemble_vote([torch.zeros(1, 9, 4, 4)], (0,))           # C > 8
    with pytest.raises(ValueError):
        ensemble_vote([torch.zeros(1, 1, 4, 4)], (0,))           # C < 2


@pytest.mark.parametrize('idx', range(len(ec.CASES)), ids=ec.IDS)
def test_vote_host_against_float64(idx):
    from aide_amd.inference import ensemble_vote, ensemble_vote_host
    z, codes = ec.case_logits(idx)
    want_l, want_p, gap = ec.case_reference(idx)
    print('smallest float64 top-two gap %.3e' % gap)
    assert gap > ec.MIN_GAP
    labels, probs = ensemble_vote_host(list(z), codes, probs=True)
    err = (probs.double() - want_p).abs().max().item()
    print('max |p - p64| = %.3e' % err)
    assert labels.dtype == torch.int64 and probs.dtype == torch.float32
    assert err <= ec.PROB_TOL
    assert torch.equal(labels, want_l)
    assert torch.equal(ensemble_vote_host(list(z), codes), labels)
    l2, p2 = ensemble_vote(list(z), codes, probs=True)           # CPU tensors take the host statement
    assert torch.equal(l2, labels) and torch.equal(p2, probs)


def test_vote_host_geometry_and_ties():
    """a map and its view vote like the map alone, bit for bit (p + p and the halving are exact); equal sums -> class 0"""
    from aide_amd.inference import ensemble_vote_host
    for idx, codes in ((1, range(1, 8)), (2, (2, 4, 6))):
        L = ec.case_logits(idx)[0][0]
        one_l, one_p = ensemble_vote_host([L], (0,), probs=True)
        for k in codes:
            l2, p2 = ensemble_vote_host([L, ec.view_apply(L, k).contiguous()], (0, k), probs=True)
            assert torch.equal(l2, one_l) and torch.equal(p2, one_p), k
    flat = torch.full((1, 5, 3, 3), 0.25)
    assert ensemble_vote_host([flat, flat], (0, 4)).eq(0).all()


class _Stub(torch.nn.Module):
    """logits that depend on the pixel, the view frame it is seen in and the network: class c gets w_c * x + b_c * column
    ramp.  Records the batch shapes it is called with."""

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


def test_predict_labels_member_order_and_chunks():
    from aide_amd.inference import predict_labels, predict_case, ensemble_logits, ensemble_vote_host
    g = torch.Generator().manual_seed(11)
    a, b = torch.randn(7, 3, 12, 12, generator=g), torch.randn(7, 3, 12, 12, generator=g)
    n1, n2 = _Stub(3, 1).eval(), _Stub(3, 2).eval()
    codes = (0, 4, 1, 6)
    # member i * V + j = network i under view j, each in its view frame
    z = ensemble_logits([n1, n2], a, b, views=codes)
    assert tuple(z.shape) == (8, 7, 3, 12, 12)
    assert n1.calls == [((28, 3, 12, 12),) * 2] and n2.calls == n1.calls
    with torch.no_grad():
        for i, net in enumerate((n1, n2)):
            for j, v in enumerate(codes):
                assert torch.equal(z[i * 4 + j], net(ec.view_apply(a, v), ec.view_apply(b, v)))
    want = ensemble_vote_host(list(z), codes * 2)
    # chunks of max(1, batch_size // V) slices, every slice returned, the same labels whatever the chunking
    for bs, shapes in ((16, [16, 12]), (8, [8, 8, 8, 4]), (3, [4] * 7), (64, [28])):
        n1.calls, n2.calls = [], []
        got = predict_labels([n1, n2], a, b, views=codes, batch_size=bs)
        assert [c[0][0] for c in n1.calls] == shapes and n2.calls == n1.calls, (bs, n1.calls)
        assert got.dtype == torch.int64 and torch.equal(got, want), bs
    # one network, named set; the identity view alone is the plain arg-max of the soft-max
    one = predict_labels(n1, a, b, views='flip2', batch_size=4)
    assert torch.equal(one, ensemble_vote_host(list(ensemble_logits(n1, a, b, views='flip2')), (0, 4)))
    with torch.no_grad():
        assert torch.equal(predict_labels(n1, a, b, views=(0,)), torch.softmax(n1(a, b), 1).argmax(1))
    vol, pr = predict_case([n1, n2], a, b, views=codes, probs=True, numpy=False)
    assert torch.equal(vol, want.permute(1, 2, 0)) and tuple(pr.shape) == (7, 3, 12, 12)
    assert torch.equal(pr, ensemble_vote_host(list(z), codes * 2, probs=True)[1])
    with pytest.raises(ValueError):
        predict_labels([n1, n2], a, b, views=ec.D4 + (0,))          # 18 members
    with pytest.raises(ValueError):
        predict_labels([n1, _Stub(4, 3).eval()], a, b, views='flip2')   # class counts differ
    with pytest.raises(ValueError):
        predict_labels(n1, a[..., :10], b[..., :10], views='d4')    # quarter turns of a 12 x 10 image
    n2.train()
    with pytest.raises(RuntimeError):
        predict_labels([n1, n2], a, b, views='flip2')


@pytest.fixture(scope='module')
def built():
    from aide_amd.build import build
    return build(verbose=False)


def test_header_declares_and_library_exports(built):
    from aide_amd._lib import lib, parse_header
    protos = parse_header()
    out = subprocess.run(['nm', '-D', '--defined-only', built], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name, nargs in (('aide_view_stack', 11), ('aide_ensemble_vote', 12)):
        assert name in protos and name in lib.protos and name in exported, name
        assert len(protos[name][1]) == nargs


def test_abi_rejects_bad_arguments_before_any_launch(built):
    """AIDE_ERR_ARG (-1) from both entry points with no device memory behind the pointers: nothing can have been launched"""
    from aide_amd._lib import lib
    fake = ctypes.c_void_p(4096)
    one = (ctypes.c_void_p * 16)(*([4096] * 16))

    def codes(*v):
        return (ctypes.c_int * len(v))(*v)

    def stack(x=fake, y=fake, views=codes(0), V=1, N=1, C=3, H=8, W=8):
        return lib.aide_view_stack(x, C * H * W, y, C * H * W, views, V, N, C, H, W, None)

    def vote(logits=one, views=codes(0), K=1, N=1, C=2, H=8, W=8, labels=fake, probs=None):
        return lib.aide_ensemble_vote(logits, views, K, C * H * W, N, C, H, W, labels, probs, C * H * W, None)

    assert stack(x=None) == -1 and stack(y=None) == -1 and stack(views=None) == -1
    assert stack(V=0) == -1 and stack(views=codes(*[0] * 17), V=17) == -1
    assert stack(views=codes(8)) == -1 and stack(views=codes(-1)) == -1
    assert stack(views=codes(1), H=8, W=12) == -1 and stack(views=codes(0, 7), V=2, H=12, W=8) == -1
    assert stack(N=0) == -1 and stack(H=0) == -1 and stack(N=1 << 15, C=4, H=128, W=128) == -1      # 2^31 elements
    assert vote(logits=None) == -1 and vote(labels=None) == -1 and vote(views=None) == -1
    assert vote(logits=(ctypes.c_void_p * 2)(4096, None), views=codes(0, 0), K=2) == -1
    assert vote(K=0) == -1 and vote(views=codes(*[0] * 17), K=17) == -1
    assert vote(C=1) == -1 and vote(C=lib.aide_seg_max_classes() + 1) == -1
    assert vote(views=codes(8)) == -1 and vote(views=codes(3), H=8, W=12) == -1
    assert vote(N=1 << 15, C=4, H=128, W=128) == -1
