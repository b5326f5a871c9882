"""-m gpu: the per-case evaluation on the device (aide_amd/csrc/eval3d.hip): the largest-connected-component filter equals
the CPU function byte for byte, the confusion sums equal the reference's formulas, and the per-case chain (predict_case,
evaluate_case of the comparison mirror) returns what the CPU chain returns."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _keep_cpu(v):
    from aide_amd.inference import keep_largest_connected_components
    return keep_largest_connected_components(np.asarray(v))


def _keep_dev(t):
    from aide_amd.inference import keep_largest_connected_components
    out = keep_largest_connected_components(t)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.shape == t.shape
    return out.cpu().numpy()


def _check(v, dev):
    ref = _keep_cpu(v)
    got = _keep_dev(torch.from_numpy(np.ascontiguousarray(v)).to(dev))
    assert got.dtype == ref.dtype and np.array_equal(got, ref), (v.shape, int(got.sum()), int(ref.sum()))
    return ref


def _serpentine(d0, d1, d2):
    """One component that winds through the whole volume: rows joined at alternating ends, planes joined at one corner."""
    v = np.zeros((d0, d1, d2), np.int64)
    for z in range(0, d0, 2):
        for y in range(0, d1, 2):
            v[z, y, :] = 1
            if y + 1 < d1:
                v[z, y + 1, d2 - 1 if (y // 2) % 2 == 0 else 0] = 1
        if z + 1 < d0:
            v[z + 1, d1 - 1 if d1 % 2 == 1 else d1 - 2, 0] = 1
    return v


@pytest.mark.parametrize('density', [0.05, 0.31, 0.7])
def test_lcc_random_binary(dev, density):
    rng = np.random.RandomState(int(density * 100))
    for shape in ((7, 13, 5), (33, 1, 250), (256, 256, 33)):
        _check((rng.rand(*shape) < density).astype(np.int64), dev)


def test_lcc_multiclass_and_negative(dev):
    rng = np.random.RandomState(11)
    for shape in ((7, 13, 5), (40, 37, 19), (256, 256, 33)):
        _check(rng.randint(0, 8, shape).astype(np.int64), dev)                      # 8 classes
        _check(rng.randint(-3, 4, shape).astype(np.int64), dev)                     # negatives are foreground
        v = -rng.randint(0, 3, shape).astype(np.int64)                              # max <= 0, negatives present
        assert _check(v, dev).sum() == 0
    # a negative blob larger than every positive one is the one kept (area decides; the max > 0 guard is global)
    v = np.zeros((6, 6, 6), np.int64)
    v[:, :, :3] = -2
    v[0, 0, 5] = 1
    assert _check(v, dev).sum() == 108


def test_lcc_edge_shapes(dev):
    rng = np.random.RandomState(5)
    for shape in ((1, 1, 1), (1, 7, 1), (7, 13, 5), (33, 1, 250), (1, 1, 300), (300, 1, 1), (17, 31, 16)):
        _check((rng.rand(*shape) < 0.5).astype(np.int64), dev)
        _check(np.zeros(shape, np.int64), dev)
    one = np.zeros((7, 13, 5), np.int64)
    one[3, 6, 2] = 5
    assert _check(one, dev).sum() == 1
    _check(np.ones((1, 1, 1), np.int64), dev)
    assert _keep_dev(torch.zeros(0, 4, 4, dtype=torch.int64, device=dev)).size == 0


def test_lcc_large_and_serpentine(dev):
    rng = np.random.RandomState(9)
    _check((rng.rand(512, 512, 100) < 0.31).astype(np.int64), dev)
    for shape in ((64, 64, 33), (9, 40, 70), (100, 64, 64)):
        v = _serpentine(*shape)
        ref = _check(v, dev)
        assert ref.sum() == v.sum()                                                 # one component
        v2 = v.copy()
        v2[v2.shape[0] // 2, :, :] = 0                                              # cut in two (+ what the cut leaves)
        _check(v2, dev)


def test_lcc_ties_and_permuted_order(dev):
    # two blobs of equal area: the first in raster order is kept
    v = np.zeros((9, 9, 9), np.int64)
    v[6:8, 6:8, 6:8] = 1
    v[0:2, 0:2, 4:6] = 3
    v[4, 4, 0:8] = 2
    assert _check(v, dev)[0, 0, 4] == 1
    # [S,H,W] labels with two equal blobs: first in [S,H,W] order is blob A, first in [H,W,S] order is blob B
    lab = torch.zeros(5, 8, 8, dtype=torch.int64)
    lab[0, 6:8, 6:8] = 1                           # A: slice 0, lower right
    lab[3, 0:2, 0:2] = 1                           # B: slice 3, upper left
    vol = lab.to(dev).permute(1, 2, 0)             # the reference's [H,W,S] volume, as a non-contiguous view
    assert not vol.is_contiguous()
    got = _keep_dev(vol)
    ref = _keep_cpu(lab.permute(1, 2, 0).contiguous().numpy())
    assert np.array_equal(got, ref) and got[0, 0, 3] == 1 and got[6, 6, 0] == 0
    # random non-contiguous volumes with many ties
    rng = np.random.RandomState(2)
    for s in range(3):
        lab = torch.from_numpy((rng.rand(33, 64, 48) < 0.2).astype(np.int64))
        got = _keep_dev(lab.to(dev).permute(1, 2, 0))
        assert np.array_equal(got, _keep_cpu(lab.permute(1, 2, 0).numpy()))


def test_lcc_deterministic_and_other_dtypes(dev):
    rng = np.random.RandomState(4)
    v = torch.from_numpy((rng.rand(256, 256, 33) < 0.31).astype(np.int64)).to(dev)
    a = _keep_dev(v)
    b = _keep_dev(v)
    assert a.tobytes() == b.tobytes()
    u8 = torch.from_numpy(rng.randint(0, 4, (20, 30, 10)).astype(np.uint8))
    assert np.array_equal(_keep_dev(u8.to(dev)), _keep_cpu(u8.numpy()))
    with pytest.raises(RuntimeError):
        _keep_dev(v.float())
    with pytest.raises(RuntimeError):
        _keep_dev(v[0])


def _ref_scores(p, t):
    i, f = p.reshape(-1).astype(np.int64), t.reshape(-1).astype(np.int64)
    with np.errstate(divide='ignore', invalid='ignore'):
        dice = 2 * np.sum(i * f) / (np.sum(i) + np.sum(f))
        iou = np.sum(i * f) / (np.sum(i) + np.sum(f) - np.sum(i * f))
    return dict(Dice=dice, IoU=iou, TP=np.sum(i * f), TN=np.sum((1 - i) * (1 - f)), FP=np.sum(i * (1 - f)),
                FN=np.sum((1 - i) * f))


def _same(a, b):
    for k in ('TP', 'TN', 'FP', 'FN'):
        assert int(a[k]) == int(b[k]), (k, a[k], b[k])
    for k in ('Dice', 'IoU'):
        x, y = np.float64(a[k]), np.float64(b[k])
        assert (np.isnan(x) and np.isnan(y)) or x == y, (k, x, y)


def test_case_scores_device(dev):
    from aide_amd.inference import case_scores
    rng = np.random.RandomState(8)
    sh = (64, 48, 33)
    cases = [
        ((rng.rand(*sh) < 0.3).astype(np.uint8), (rng.rand(*sh) < 0.4).astype(np.int64)),
        ((rng.rand(*sh) < 0.3).astype(np.int64), (rng.rand(*sh) < 0.4).astype(np.uint8)),
        ((rng.rand(*sh) < 0.3).astype(np.uint8), (rng.rand(*sh) < 0.4).astype(np.uint8)),
        (rng.randint(0, 5, sh).astype(np.int64), rng.randint(0, 3, sh).astype(np.int64)),             # non-binary
        (rng.randint(-4, 5, sh).astype(np.int64), rng.randint(-2, 3, sh).astype(np.int64)),
        (np.zeros(sh, np.uint8), (rng.rand(*sh) < 0.5).astype(np.int64)),                           # empty prediction
        (np.zeros(sh, np.int64), np.zeros(sh, np.int64)),                                           # 0/0 -> nan
        ((rng.rand(256, 256, 33) < 0.5).astype(np.uint8), (rng.rand(256, 256, 33) < 0.5).astype(np.int64)),
        ((rng.rand(7, 1) < 0.5).astype(np.int64), (rng.rand(7, 1) < 0.5).astype(np.int64)),         # 2-D
    ]
    for p, t in cases:
        ref = _ref_scores(p, t)
        host = case_scores(p, t)
        devs = case_scores(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev))
        _same(host, ref)
        _same(devs, ref)
    # strided operands: [S,H,W] views as [H,W,S]
    p = torch.from_numpy((rng.rand(33, 64, 64) < 0.3).astype(np.int64))
    t = torch.from_numpy((rng.rand(33, 64, 64) < 0.3).astype(np.uint8))
    _same(case_scores(p.to(dev).permute(1, 2, 0), t.to(dev).permute(1, 2, 0)),
          _ref_scores(p.permute(1, 2, 0).numpy(), t.permute(1, 2, 0).numpy()))
    with pytest.raises(RuntimeError):
        case_scores(p.to(dev), t.to(dev).permute(1, 2, 0))


def _trained(dev, name):
    from aide_amd import utils as U
    from aide_amd.models_singlemodalinput import UNet
    from aide_amd.models_twomodalinputs import fuseunet
    from aide_amd.optim import Adam
    two = name == 'fuseunet'
    g = torch.Generator().manual_seed(1234)
    xs = [torch.randn(2, 3, 32, 32, generator=g).to(dev) for _ in range(2 if two else 1)]
    t = (torch.rand(2, 32, 32, generator=g) > 0.7).long().to(dev)
    torch.manual_seed(2)
    net = (fuseunet(2) if two else UNet(2)).to(dev)
    net.train()
    w = torch.tensor([1.0, 1.0])
    crit = U.CEMDiceLoss(cediceweight=w, ceclassweight=w, diceclassweight=w)
    opt = Adam(net.parameters(), lr=1e-4, amsgrad=True)
    for _ in range(2):
        opt.zero_grad()
        crit(net(*xs), t).backward()
        opt.step()
    net.eval()
    return net, two


@pytest.mark.parametrize('name', ['fuseunet', 'unet'])
def test_predict_case_keep_largest(dev, name):
    from aide_amd.inference import predict_case, keep_largest_connected_components
    net, two = _trained(dev, name)
    g = torch.Generator().manual_seed(77)
    sl = [torch.randn(6, 3, 48, 32, generator=g) for _ in range(2 if two else 1)]
    vol = predict_case(net, *sl, batch_size=4)
    ref = keep_largest_connected_components(vol)
    got = predict_case(net, *sl, batch_size=4, keep_largest=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, ref)
    d = predict_case(net, *sl, batch_size=4, keep_largest=True, numpy=False)
    assert d.is_cuda and np.array_equal(d.cpu().numpy(), ref)
    raw = predict_case(net, *sl, batch_size=4, numpy=False)
    assert raw.is_cuda and tuple(raw.shape) == vol.shape and np.array_equal(raw.cpu().numpy(), vol)


@pytest.mark.parametrize('name', ['fuseunet', 'UNet'])
def test_evaluate_case_matches_cpu_chain(dev, name):
    """evaluate_case (device filter + device sums) returns exactly the value of the former CPU chain."""
    from aide_amd.inference import predict_case, Dice3d_fn, keep_largest_connected_components
    from aide_amd.synthetic import chaos_batch
    from aide_amd.train_files.trainchaos_comparison_1case import evaluate_case, parse_args
    net, two = _trained(dev, 'fuseunet' if name == 'fuseunet' else 'unet')
    single = not two
    for seed, size in ((2, 64), (5, 96)):
        args = parse_args(['--model_name', name, '--torch_seed', str(seed), '--img_size', str(size)])
        got = evaluate_case(net, args, dev, single, 0)
        assert net.training
        net.eval()
        inphase, outphase, targets = chaos_batch(8, size, seed=seed * 7919 + 13, single_modal=single)
        mods = (inphase,) if single else (inphase, outphase)
        pred = keep_largest_connected_components(predict_case(net, *mods, batch_size=8))
        tgt = targets.permute(1, 2, 0).contiguous().numpy()
        want = 1.0 if tgt.sum() == 0 and pred.sum() == 0 else float(Dice3d_fn(pred, tgt))
        assert type(got) is float and (got == want or (np.isnan(got) and np.isnan(want))), (got, want)
