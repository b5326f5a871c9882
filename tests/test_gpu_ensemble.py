"""-m gpu: test-time augmentation on the device (aide_amd/csrc/ensemble.hip, aide_amd/ensemble.py).  `aide_view_stack` is the
torch flip / rot90 stack byte for byte; `aide_ensemble_vote` meets the float64 statement on the five cases of ensemble_cases
(probabilities within PROB_TOL, labels equal at every pixel: the cases' float64 top-two gaps exceed MIN_GAP) and repeats its
bytes from call to call; a map voted together with one of its own views gives the bits of the map alone (p + p and the
halving are exact), which fails on a wrong inverse view or a wrong tile edge; one member under the identity is `label_map`,
first-maximum rule included; and `predict_labels(..., views=...)` and its callers equal the chain composed from these parts.
The device soft-max is not asserted byte-equal to `ensemble_vote_host`: the exponentials of the two libraries differ."""
import ctypes

import pytest
import torch

import ensemble_cases as ec

pytestmark = pytest.mark.gpu


def close(a, b, rtol=1e-3, what=''):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs().max().item()
    assert err <= rtol * (b.abs().max().item() + 1e-12) + 1e-9, '%s: err %.3e (scale %.3e)' % (what, err, b.abs().max().item())


@pytest.mark.parametrize('shape', sorted(set(ec.SHAPES)), ids=lambda s: '%dx%dx%d' % s)
def test_view_stack_is_the_torch_stack(dev, shape):
    from aide_amd.inference import view_stack
    n, h, w = shape
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + w)
    x = torch.randn(n, 3, h, w, generator=g)
    codes = ec.valid_codes(h, w)
    for views in (codes, codes[::-1] + codes[:1], codes[-1:]):          # every valid code; a duplicate; a single view
        want = torch.stack([ec.view_apply(x, v) for v in views])
        got = view_stack(x.to(dev), views)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got.cpu(), want), views
    # a non-contiguous input is read through a contiguous copy
    assert torch.equal(view_stack(x.to(dev).transpose(0, 1), codes[:2]).cpu(),
                       torch.stack([ec.view_apply(x.transpose(0, 1), v) for v in codes[:2]]))


@pytest.mark.parametrize('idx', range(len(ec.CASES)), ids=ec.IDS)
def test_vote_against_float64(dev, idx):
    from aide_amd.inference import ensemble_vote
    z, codes = ec.case_logits(idx)
    want_l, want_p, gap = ec.case_reference(idx)
    assert gap > ec.MIN_GAP
    zd = z.to(dev)
    labels, probs = ensemble_vote(list(zd), codes, probs=True)
    assert labels.is_cuda and labels.dtype == torch.int64 and probs.dtype == torch.float32
    err = (probs.cpu().double() - want_p).abs().max().item()
    print('max |p - p64| = %.3e (gap %.3e)' % (err, gap))
    assert err <= ec.PROB_TOL
    assert torch.equal(labels.cpu(), want_l)
    l2, p2 = ensemble_vote(list(zd), codes, probs=True)                 # the same bytes from call to call
    assert torch.equal(l2, labels) and torch.equal(p2, probs)
    assert torch.equal(ensemble_vote(list(zd), codes), labels)          # without the probabilities
    # members that are separate tensors, not slices of one stack
    assert torch.equal(ensemble_vote([m.clone() for m in zd], codes), labels)


@pytest.mark.parametrize('idx', range(len(ec.CASES)), ids=ec.IDS)
def test_vote_geometry_exact(dev, idx):
    from aide_amd.inference import ensemble_vote, label_map
    L = ec.case_logits(idx)[0][0]
    h, w = L.shape[-2:]
    Ld = L.to(dev)
    one_l, one_p = ensemble_vote([Ld], (0,), probs=True)
    assert torch.equal(one_l, label_map(Ld))
    for k in ec.valid_codes(h, w)[1:]:
        M = ec.view_apply(L, k).contiguous().to(dev)
        l2, p2 = ensemble_vote([Ld, M], (0, k), probs=True)
        assert torch.equal(p2, one_p), 'view %d: %d pixels differ' % (k, int((p2 != one_p).any(1).sum()))
        assert torch.equal(l2, one_l), k
        l1, p1 = ensemble_vote([M], (k,), probs=True)                   # the viewed map alone
        assert torch.equal(p1, one_p) and torch.equal(l1, one_l), k


@pytest.mark.parametrize('C', [2, 5])
def test_one_member_identity_is_label_map(dev, C):
    from aide_amd.inference import ensemble_vote, label_map
    g = torch.Generator().manual_seed(40 + C)
    z = (3 * torch.randn(3, C, 37, 45, generator=g)).to(dev)
    z[0, :, :5] = z[0, :1, :5]                                          # exact ties of every class: the first wins
    z[1, C - 1, 7] = z[1, 0, 7] = 50.0                                  # the first and the last class tie for the largest
    want = label_map(z)
    assert torch.equal(ensemble_vote([z], (0,)), want)
    assert want[0, :5].eq(0).all() and want[1, 7].eq(0).all()
    flat = torch.full((2, C, 33, 9), 0.5, device=dev)
    labels, probs = ensemble_vote([flat, flat, flat], (0, 4, 2), probs=True)
    assert labels.eq(0).all() and torch.equal(labels, label_map(flat))
    assert (probs.cpu().double() - 1.0 / C).abs().max().item() <= ec.PROB_TOL


def test_bad_arguments_launch_nothing(dev):
    from aide_amd._lib import lib
    from aide_amd.ops import ptr, stream_ptr
    from aide_amd.inference import ensemble_vote, view_stack
    z = torch.zeros(1, 2, 8, 12, device=dev)
    for members, views in (([z], (1,)), ([z, z], (0, 7)), ([z], (8,)), ([z], ()), ([z, z], (0,)), ([z] * 17, (0,) * 17),
                           ([z, z[:, :, :, :8]], (0, 0)), ([z, z.double()], (0, 0)), ([z[0]], (0,))):
        with pytest.raises(ValueError):
            ensemble_vote(members, views)
    for views in ('d4', (3,), (), (9,), (0,) * 17):
        with pytest.raises(ValueError):
            view_stack(z, views)
    # the C ABI itself, with real device memory: refused, and the outputs keep their bytes
    labels = torch.full((1, 8, 12), -7, device=dev, dtype=torch.int64)
    y = torch.full((1, 1, 2, 8, 12), -7.0, device=dev)
    arr = (ctypes.c_void_p * 1)(z.data_ptr())
    for code, c in ((1, 2), (8, 2), (0, 9), (0, 1)):
        va = (ctypes.c_int * 1)(code)
        assert lib.aide_ensemble_vote(arr, va, 1, 192, 1, c, 8, 12, ptr(labels), None, 192, stream_ptr()) == -1
    for code in (1, 3, 8, -1):
        va = (ctypes.c_int * 1)(code)
        assert lib.aide_view_stack(ptr(z), 192, ptr(y), 192, va, 1, 1, 2, 8, 12, stream_ptr()) == -1
    torch.cuda.synchronize()
    assert labels.eq(-7).all() and y.eq(-7.0).all()


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


@pytest.mark.parametrize('kind,classes,hw,views', [('UNet', 2, (32, 32), 'd4'), ('fuseunet', 2, (32, 32), 'd4'),
                                                   ('UNet', 3, (48, 32), 'flip4')], ids=['unet-d4', 'fuseunet-d4', 'unet3-flip4'])
def test_predict_labels_equals_its_parts(dev, kind, classes, hw, views):
    from aide_amd.inference import ensemble_logits, ensemble_vote, predict_labels, predict_case, view_codes, \
        keep_largest_connected_components
    net = _net(dev, kind, classes)
    xs = _inputs(dev, kind, 3, *hw)
    codes = view_codes(views, *hw)
    V = len(codes)
    z = ensemble_logits(net, *xs, views=views)
    assert tuple(z.shape) == (V, 3, classes) + hw
    with torch.no_grad():
        for j, v in enumerate(codes):                                   # member j = the network under view j, in its frame
            close(z[j], net(*[ec.view_apply(x, v).contiguous() for x in xs]), rtol=1e-3, what='view %d' % v)
    want = ensemble_vote(list(z), codes)
    got = predict_labels(net, *xs, views=views, batch_size=3 * V)       # one forward batch, as ensemble_logits ran it
    assert got.dtype == torch.int64 and tuple(got.shape) == (3,) + hw and torch.equal(got, want)
    # the identity view alone: today's path, byte for byte
    assert torch.equal(predict_labels(net, *xs, views=(0,)), predict_labels(net, *xs))
    # batch_size below V: one slice (V images) per forward, every slice returned
    small = predict_labels(net, *xs, views=views, batch_size=2)
    per_slice = torch.cat([ensemble_vote(list(ensemble_logits(net, *[x[i:i + 1] for x in xs], views=views)), codes)
                           for i in range(3)])
    assert tuple(small.shape) == (3,) + hw and torch.equal(small, per_slice)
    # predict_case: the filtered volume of the voted labels, and the mean probabilities on request
    vol = predict_case(net, *xs, views=views, keep_largest=True, numpy=False, batch_size=3 * V)
    assert vol.dtype == torch.uint8 and torch.equal(vol, keep_largest_connected_components(want.permute(1, 2, 0)))
    vol2, pr = predict_case(net, *xs, views=views, probs=True, numpy=False, batch_size=3 * V)
    assert torch.equal(vol2, want.permute(1, 2, 0)) and torch.equal(pr, ensemble_vote(list(z), codes, probs=True)[1])
    assert predict_case(net, *xs, views=views, batch_size=3 * V).shape == hw + (3,)


def test_two_networks_vote_together(dev):
    from aide_amd.inference import ensemble_logits, ensemble_vote, predict_labels
    nets = [_net(dev, 'UNet', 2, seed=5), _net(dev, 'UNet', 2, seed=6)]
    (x,) = _inputs(dev, 'UNet', 2, 32, 32)
    z = ensemble_logits(nets, x, views='flip2')
    assert tuple(z.shape) == (4, 2, 2, 32, 32)
    for i, net in enumerate(nets):                                      # member i * V + j = network i under view j
        assert torch.equal(z[2 * i:2 * i + 2], ensemble_logits(net, x, views='flip2'))
    got = predict_labels(nets, x, views='flip2', batch_size=4)
    assert torch.equal(got, ensemble_vote(list(z), (0, 4, 0, 4)))
    assert not torch.equal(z[0], z[2])
    with pytest.raises(ValueError):
        predict_labels(nets + nets + [nets[0]], x, views='flip4')       # K = 20
    nets[1].train()
    with pytest.raises(RuntimeError):
        predict_labels(nets, x, views='flip2')
    nets[1].eval()


def test_bank_refresh_with_views(dev):
    from aide_amd.inference import predict_labels, evaluate_cases, evaluate_label_maps
    from aide_amd.labelbank import PseudoLabelBank
    from aide_amd.synthetic import chaos_cases
    nets = [_net(dev, 'fuseunet', 2, seed=5), _net(dev, 'fuseunet', 2, seed=6)]
    cs = chaos_cases(8, 32, seed=3, slices=(1, 4), labelled=(0, 5))
    inputs = (cs['inphase'].to(dev), cs['outphase'].to(dev))
    a = PseudoLabelBank(cs['initial'].to(dev), cs['slice_start'], cs['labelled'])
    b = PseudoLabelBank(cs['initial'].to(dev), cs['slice_start'], cs['labelled'])
    labels = [predict_labels(net, *inputs, views='flip2', batch_size=4) for net in nets]
    assert a.refresh(nets[0], nets[1], inputs, 0, 1, batch_size=4, views='flip2')
    assert b.refresh_from_labels(labels[0], labels[1], 0, 1)
    assert torch.equal(a.bank, b.bank) and torch.equal(a.rank, b.rank) and torch.equal(a.selected, b.selected)
    assert torch.equal(a.case_dice().view(torch.int32), b.case_dice().view(torch.int32))
    st = torch.tensor(cs['slice_start'], dtype=torch.int64, device=dev)
    plane = cs['initial'].to(dev)
    r = evaluate_cases(nets[0], inputs, st, plane, batch_size=4, views='flip2')
    w = evaluate_label_maps(labels[0], st, plane)
    assert all(torch.equal(r[k], w[k]) for k in ('filtered', 'sums', 'rank', 'selected'))
    assert torch.equal(r['dice'].view(torch.int32), w['dice'].view(torch.int32))
