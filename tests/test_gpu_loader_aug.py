"""-m gpu: the proposed loaders' transform chain on the device (aide_amd/csrc/augment.hip, utils/loader_aug.py) against the
reference's own transform.py (fixture g22) and against PIL directly: u8 stages bit-exact, float outputs to the reduction
order of torch's mean / std; the forward views undone exactly by the existing reverse-augmentation kernel; stream
ordering without host synchronisation; and the proposed loop with DEVICE_AUGMENT on."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _g22():
    return np.load(os.path.join(GOLD, 'g22_loader_aug.npz'))


def _params(fx, key):
    n = int(fx['%s/meta' % key][0])
    p = {'augno': [4] * n}
    for k in range(4):
        p['degree%d' % (k + 1)] = [float(v) for v in fx['%s/degree' % key][k]]
        p['hflip%d' % (k + 1)] = [int(v) for v in fx['%s/hflip' % key][k]]
    return p


def _run_case(fx, key, dev):
    from aide_amd.utils.loader_aug import LoaderAugment
    n, M, S, _, floats = [int(v) for v in fx['%s/meta' % key]]
    imgs = [tuple(fx['%s/src%d_%d' % (key, i, m)] for m in range(M)) for i in range(n)]
    masks = [fx['%s/mask%d' % (key, i)] for i in range(n)]
    mean = fx['%s/mean' % key] if '%s/mean' % key in fx.files else None
    std = fx['%s/std' % key] if '%s/std' % key in fx.files else None
    aug = LoaderAugment(S, float(fx['%s/rotation' % key]), mean, std)
    return aug(imgs if M > 1 else [i[0] for i in imgs], _params(fx, key), masks=masks, raw=not floats, device=dev), M, floats


def test_g22_reference_chain(dev):
    fx = _g22()
    for key in fx['cases']:
        (base, augset, onehot), M, floats = _run_case(fx, key, dev)
        for m in range(M):
            outs = [(base[m], fx['%s/base%d' % (key, m)])]
            for k in range(1, 5):
                name = ('imgmodal%d%d' % (m + 1, k)) if M > 1 else ('img%d' % k)
                outs.append((augset[name], fx['%s/view%d_%d' % (key, m, k)]))
            for j, (got, ref) in enumerate(outs):
                got = got.cpu().numpy()
                assert got.shape == ref.shape and got.dtype == ref.dtype, (key, m, j, got.shape, ref.shape)
                if floats:
                    err = np.abs(got.astype(np.float64) - ref) / (1.0 + np.abs(ref))
                    assert err.max() <= 2e-6, (key, m, j, err.max())
                else:
                    assert np.array_equal(got, ref), (key, m, j, int((got != ref).sum()))
        if '%s/onehot' % key in fx.files:
            assert onehot[0].dtype == torch.int64
            assert np.array_equal(onehot[0].cpu().numpy(), fx['%s/onehot' % key].astype(np.int64)), key


def _pil_view(a, S, deg, flip):
    im = Image.fromarray(a).convert('RGB').resize((S, S), Image.BILINEAR).rotate(deg, Image.BILINEAR)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.array(im)[:, :, 0]


def test_views_match_pil_sweep(dev):
    """every u8 view bit-exact with PIL: special and random angles, both flips, square / non-square / odd / tiny planes,
    up and down resize, u16 clamp"""
    from aide_amd.utils.loader_aug import LoaderAugment
    rng = np.random.RandomState(5)
    pr = random.Random(9)
    rot = 60.0
    angles = [0.0, 90.0, 180.0, 270.0, -90.0, 360.0, rot, -rot] + [pr.uniform(-180, 180) for _ in range(20)]
    shapes = [((64, 64), 64), ((48, 80), 64), ((97, 101), 64), ((288, 288), 256), ((200, 232), 256), ((5, 7), 9),
              ((3, 3), 2), ((31, 29), 33), ((20, 20), 64)]
    for si, ((h, w), S) in enumerate(shapes):
        u16 = si % 3 == 1
        imgs = [rng.randint(0, 700 if u16 else 256, (h, w)).astype(np.uint16 if u16 else np.uint8) for _ in range(len(angles) // 4)]
        p = {'augno': [4] * len(imgs)}
        for k in range(4):
            p['degree%d' % (k + 1)] = [angles[i * 4 + k] for i in range(len(imgs))]
            p['hflip%d' % (k + 1)] = [(i + k + si) % 2 for i in range(len(imgs))]
        base, augset, _ = LoaderAugment(S, rot)(imgs, p, raw=True, device=dev)
        for i, a in enumerate(imgs):
            ref0 = _pil_view(a, S, 0.0, 0)
            assert np.array_equal(base[0][i].cpu().numpy(), ref0), (h, w, S, 'base')
            for k in range(4):
                deg, fl = p['degree%d' % (k + 1)][i], p['hflip%d' % (k + 1)][i]
                got = augset['img%d' % (k + 1)][i].cpu().numpy()
                ref = _pil_view(a, S, deg, fl)
                assert np.array_equal(got, ref), (h, w, S, deg, fl, int((got != ref).sum()))


def test_round_trip_with_reverse_aug(dev):
    """forward view (rotate, then flip) undone by reverse_aug_tensor (flip, then rotate by -deg): the base comes back exactly"""
    from aide_amd.utils.loader_aug import LoaderAugment
    from aide_amd.utils.augment import reverse_aug_tensor
    rng = np.random.RandomState(1)
    degs = [0.0, 90.0, 180.0, 270.0]
    for flip in (0, 1):
        imgs = [rng.randint(0, 256, (40, 40)).astype(np.uint8) for _ in range(4)]
        p = {'augno': [4] * 4}
        for k in range(4):
            p['degree%d' % (k + 1)] = [degs[(i + k) % 4] for i in range(4)]
            p['hflip%d' % (k + 1)] = [flip] * 4
        base, augset, _ = LoaderAugment(32, 60.0)(imgs, p, raw=True, device=dev)
        ref = base[0].float().unsqueeze(1)
        for k in range(4):
            v = augset['img%d' % (k + 1)].float().unsqueeze(1).contiguous()
            back = reverse_aug_tensor(v, p['hflip%d' % (k + 1)], p['degree%d' % (k + 1)])
            assert torch.equal(back, ref), (flip, k)


def test_stream_order_no_sync(dev):
    """same result on a side stream; no host synchronisation on the path; one call of each launching entry point per batch
    (the kernels themselves are counted by test_kernel_launches_per_batch)"""
    from aide_amd import _lib
    from aide_amd.utils.loader_aug import LoaderAugment, draw_aug_params
    from aide_amd.synthetic import chaos_slice
    r = np.random.RandomState(4)
    sl = [chaos_slice(r, 64) for _ in range(4)]
    imgs = [(s[0], s[1]) for s in sl]
    masks = [(s[2] * 63).astype(np.uint8) for s in sl]
    p = draw_aug_params(4, 60.0, random.Random(2))
    aug = LoaderAugment(64, 60.0)
    b0, a0, m0 = aug(imgs, p, masks=masks, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    saved = _lib.COVER
    _lib.COVER = {}
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            with torch.cuda.stream(side):
                b1, a1, m1 = aug(imgs, p, masks=masks, device=dev)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        calls = dict(_lib.COVER)
    finally:
        _lib.COVER = saved
    assert calls == {'aide_loader_aug_ws_bytes': 1, 'aide_loader_aug': 1, 'aide_loader_mask_onehot': 1}, calls
    side.synchronize()
    for x, y in zip(b0, b1):
        assert torch.equal(x, y)
    for k in range(1, 5):
        for m in (1, 2):
            assert torch.equal(a0['imgmodal%d%d' % (m, k)], a1['imgmodal%d%d' % (m, k)])
    assert torch.equal(m0[0], m1[0])


def test_proposed_loop_with_device_augment(dev, monkeypatch):
    from aide_amd.train_files import trainchaos_proposed_30cases1labeled as mod
    losses = []
    step = mod.coteach_step

    def rec(*a, **k):
        r = step(*a, **k)
        losses.append((r['loss1'], r['loss2']))
        return r
    monkeypatch.setattr(mod, 'coteach_step', rec)
    monkeypatch.setattr(mod, 'DEVICE_AUGMENT', [True])
    # (batch 4, the reference's: with batch 2 the loss keeps both images of the batch and is NaN on the default path too)
    args = mod.parse_args(['--batch_size', '4', '--img_size', '64', '--num_epoch', '1', '--steps_per_epoch', '2',
                           '--warmup_epoch', '2', '--checkpoint', ''])
    n1, n2 = mod.Train(args)
    assert len(losses) == 2
    assert all(torch.isfinite(l).all() for pair in losses for l in pair)
    assert all(torch.isfinite(p).all() for p in list(n1.parameters()) + list(n2.parameters()))


def test_coteach_step_device_views_vs_host_chain(dev):
    """coteach_step fed with the device views selects the same images, with the same losses (1e-5), as fed with the
    reference host chain's views (g22) uploaded"""
    from aide_amd.models_twomodalinputs import fuseunet
    from aide_amd.optim import Adam
    from aide_amd.utils import CoTeachingProposedLoss
    from aide_amd.train_files.trainchaos_proposed_30cases1labeled import coteach_step
    fx = _g22()
    key = 'chaos_f32'
    (base, augset, onehot), M, _ = _run_case(fx, key, dev)
    t = (onehot[0][:, 0] == 0).long()                        # foreground: every pixel not of palette value 0
    host = {'b%d' % m: torch.from_numpy(fx['%s/base%d' % (key, m)]).to(dev) for m in range(2)}
    hv = [tuple(torch.from_numpy(fx['%s/view%d_%d' % (key, m, k)]).to(dev) for m in range(2)) for k in range(1, 5)]
    dv = [(augset['imgmodal1%d' % k], augset['imgmodal2%d' % k]) for k in range(1, 5)]
    res = []
    for xin, xout, views in ((base[0], base[1], dv), (host['b0'], host['b1'], hv)):
        torch.manual_seed(3)
        n1, n2 = fuseunet(2).to(dev), fuseunet(2).to(dev)
        o1, o2 = Adam(n1.parameters(), lr=1e-4, amsgrad=True), Adam(n2.parameters(), lr=1e-4, amsgrad=True)
        op = CoTeachingProposedLoss(cediceweight=[1.0, 1.0], ceclassweight=[1.0, 1.0], segcor_weight=[1.0, 10.0], keep=1)
        aug = {kk: v for kk, v in augset.items() if not kk.startswith('imgmodal') and not kk.startswith('_')}
        r = coteach_step(n1, n2, o1, o2, op, xin.contiguous(), xout.contiguous(), views, t, t, 0.5, 1.0, augset=aug)
        torch.cuda.synchronize()
        res.append(r)
    a, b = res
    for k in ('indx1', 'indx2'):
        assert torch.equal(torch.as_tensor(a[k]).cpu(), torch.as_tensor(b[k]).cpu()), k
    for k in ('loss1', 'loss2'):
        assert abs(a[k].item() - b[k].item()) <= 1e-5 * (1 + abs(b[k].item())), (k, a[k].item(), b[k].item())


def test_several_masks_per_sample(dev):
    """N = 3 samples with Q = 3 masks each, every mask of its own size: one-hot [N, 5, S, S] per mask index equals PIL
    NEAREST + dataset.py's one_hot_mask (values outside the palette: all-zero rows)"""
    from aide_amd.utils.loader_aug import LoaderAugment, draw_aug_params, CHAOS_PALETTE
    rng = np.random.RandomState(12)
    S, N, Q = 40, 3, 3
    imgs = [rng.randint(0, 256, (30 + n, 36)).astype(np.uint8) for n in range(N)]
    pal = np.asarray(CHAOS_PALETTE + (100,), np.uint8)
    masks = [tuple(pal[rng.randint(0, 6, (20 + 7 * q + 3 * n, 50 - 6 * q + n))] for q in range(Q)) for n in range(N)]
    _, _, onehot = LoaderAugment(S, 60.0)(imgs, draw_aug_params(N, 60.0, random.Random(4)), masks=masks, device=dev)
    assert len(onehot) == Q
    for q in range(Q):
        got = onehot[q].cpu().numpy()
        assert got.shape == (N, len(CHAOS_PALETTE), S, S) and got.dtype == np.int64
        for n in range(N):
            r = np.array(Image.fromarray(masks[n][q]).resize((S, S), Image.NEAREST))
            ref = np.stack([(r == c).astype(np.int64) for c in CHAOS_PALETTE])
            assert np.array_equal(got[n], ref), (q, n)


def test_kernel_launches_per_batch(dev):
    """the kernel timer counts the launches themselves: 2 for the images, 1 more with masks"""
    from aide_amd.profiling import DispatchTimer
    from aide_amd.utils.loader_aug import LoaderAugment, draw_aug_params
    rng = np.random.RandomState(2)
    imgs = [(rng.randint(0, 256, (64, 64)).astype(np.uint8), rng.randint(0, 256, (70, 60)).astype(np.uint8))
            for _ in range(4)]
    masks = [rng.randint(0, 2, (64, 64)).astype(np.uint8) * 63 for _ in range(4)]
    p = draw_aug_params(4, 60.0, random.Random(3))
    aug = LoaderAugment(64, 60.0)
    aug(imgs, p, masks=masks, device=dev)             # (warm: tables cached, pinned block allocated)
    torch.cuda.synchronize()
    counts = []
    for mk in (None, masks):
        timer = DispatchTimer(16, families=[15])      # family 15: the kernels of augment.hip (and other small ones)
        timer.start()
        try:
            aug(imgs, p, masks=mk, device=dev)
        finally:
            timer.stop()
        counts.append(len(timer.timeline()))
    assert counts == [2, 3], counts


def test_reverseaug_cached_rows_equal_uploaded_rows(dev):
    """reverseaug on LoaderAugment's augset (rotation rows uploaded with the views) gives the same bytes as with the rows
    built and uploaded by reverseaug itself"""
    from aide_amd.utils import reverseaug
    from aide_amd.utils.loader_aug import LoaderAugment, draw_aug_params
    rng = np.random.RandomState(6)
    S, N = 48, 4
    imgs = [(rng.randint(0, 256, (50, 44)).astype(np.uint8), rng.randint(0, 256, (50, 44)).astype(np.uint8))
            for _ in range(N)]
    p = draw_aug_params(N, 60.0, random.Random(7))
    p['degree2'][0], p['degree3'][1], p['hflip2'][0] = 90.0, 180.0, 1      # the transpose paths as well
    _, augset, _ = LoaderAugment(S, 60.0)(imgs, p, device=dev)
    assert '_aide_revpar' in augset
    g = torch.Generator(device='cpu').manual_seed(0)
    logits = [torch.randn(N, 2, S, S, generator=g).to(dev) for _ in range(4)]
    cached = reverseaug(augset, [x.clone() for x in logits], 2)
    plain = reverseaug({k: v for k, v in augset.items() if k != '_aide_revpar'}, [x.clone() for x in logits], 2)
    for a, b in zip(cached, plain):
        assert torch.equal(a, b)
    with pytest.raises(AssertionError):
        reverseaug(augset, [x.clone() for x in logits], 3)
