"""Writes tests/golden/g22_loader_aug.npz: the proposed loaders' transform chain as the reference runs it.

    python tools/gen_golden_loader_aug.py

The reference's transform.py files (datasetchaos_proposed/, datasetkidney_proposed/) are loaded by path (their packages'
__init__ import pydicom and pandas) and their Compose([Resize, RandomRotate, RandomHorizontallyFlip, ToTensor, Normalize])
runs under a seeded `random`, one sample after another as a loader worker does; dataset.py's one_hot_mask comes through
oracle.gen_golden._ref_functions.  Per case the file holds the source planes, the drawn angles / flips and the outputs:
the u8 views of the chain without ToTensor / Normalize (same seed, same draws) for 256 x 256 outputs, and the float32
tensors of the whole chain for small outputs."""
import importlib.util
import os
import random
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF, _ref_functions  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'g22_loader_aug.npz')
PALETTE = [[0], [63], [126], [189], [252]]


def _load(name, sub):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, sub, 'transform.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def smooth_plane(rng, h, w, hi=255, noise=0):
    """a smooth field with a disc and optional light noise"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = 0.5 + 0.3 * np.sin(xx / (5 + 10 * rng.rand()) + rng.rand() * 6) * np.cos(yy / (4 + 9 * rng.rand()))
    f += 0.25 * (((yy - h * rng.uniform(0.3, 0.7)) / (0.3 * h)) ** 2 + ((xx - w * rng.uniform(0.3, 0.7)) / (0.25 * w)) ** 2 < 1)
    return np.clip(f * hi + rng.randint(-noise, noise + 1, (h, w)), 0, hi).astype(np.uint16 if hi > 255 else np.uint8)


def block_plane(rng, h, w, hi=255):
    """piecewise-constant 16 x 16 blocks with a disc: after rotation mostly flat, so the 256 x 256 views compress well"""
    f = rng.randint(0, hi + 1, ((h + 15) // 16, (w + 15) // 16)).astype(np.float64)
    f = np.kron(f, np.ones((16, 16)))[:h, :w]
    yy, xx = np.mgrid[0:h, 0:w]
    f[((yy - h / 2) / (0.3 * h)) ** 2 + ((xx - w / 2) / (0.25 * w)) ** 2 < 1] = hi * 0.9
    return f.astype(np.uint16 if hi > 255 else np.uint8)


def mask_plane(rng, h, w):
    """CHAOS palette values in blocks, plus a few values outside the palette"""
    m = np.asarray([0, 63, 126, 189, 252], np.uint8)[rng.randint(0, 5, ((h + 7) // 8, (w + 7) // 8))]
    m = np.kron(m, np.ones((8, 8), np.uint8))[:h, :w].copy()
    m[rng.rand(h, w) < 0.02] = 100
    return m


def run_case(out, key, T, two_modal, planes, masks, size, rotation, seed, floats, mean=None, std=None):
    """planes: per sample a list of source arrays (1 or 2 modalities); masks: per sample one u8 mask"""
    one_hot_mask, = _ref_functions(os.path.join(REF, 'datasetchaos_proposed', 'dataset.py'), ['one_hot_mask'], dict(np=np))
    chain = [T.Resize((size, size)), T.RandomRotate(rotation), T.RandomHorizontallyFlip()]
    if floats:
        chain += [T.ToTensor(), T.Normalize(mean, std)]
    comp = T.Compose(chain)
    random.seed(seed)
    res = []
    for n, src in enumerate(planes):
        imgs = [Image.fromarray(a).convert('RGB') for a in src]
        mk = Image.fromarray(masks[n])
        if two_modal:
            augset = {'augno': 4}
            for k in range(1, 5):
                augset.update({'imgmodal1%d' % k: imgs[0].copy(), 'imgmodal2%d' % k: imgs[1].copy(),
                               'degree%d' % k: 0.0, 'hflip%d' % k: 0})
            i1, i2, augset, m0, _, _ = comp(imgs[0], imgs[1], augset, mk, mk.copy(), mk.copy())
            base = [i1, i2]
        else:
            augset = {'augno': 4}
            for k in range(1, 5):
                augset.update({'img%d' % k: imgs[0].copy(), 'degree%d' % k: 0.0, 'hflip%d' % k: 0})
            i1, augset, m0, _, _ = comp(imgs[0], augset, mk, mk.copy(), mk.copy())
            base = [i1]
        # (the kidney loader's ToTensor rescales its masks to class indices: out of scope, only the chaos one-hot is kept)
        oh = one_hot_mask(np.expand_dims(np.array(m0), axis=2), PALETTE).transpose([2, 0, 1]) if two_modal else None
        res.append((base, augset, oh))
        for m, a in enumerate(src):
            out['%s/src%d_%d' % (key, n, m)] = a
        out['%s/mask%d' % (key, n)] = masks[n]
    N, M = len(planes), len(planes[0])

    def arr(x):
        return x.numpy() if floats else np.array(x)[:, :, 0]
    for m in range(M):
        out['%s/base%d' % (key, m)] = np.stack([arr(r[0][m]) for r in res])
        for k in range(1, 5):
            name = ('imgmodal%d%d' % (m + 1, k)) if two_modal else ('img%d' % k)
            out['%s/view%d_%d' % (key, m, k)] = np.stack([arr(r[1][name]) for r in res])
    out['%s/degree' % key] = np.asarray([[r[1]['degree%d' % k] for r in res] for k in range(1, 5)], np.float64)
    out['%s/hflip' % key] = np.asarray([[r[1]['hflip%d' % k] for r in res] for k in range(1, 5)], np.int64)
    if two_modal:
        out['%s/onehot' % key] = np.stack([r[2] for r in res]).astype(np.uint8)
    out['%s/meta' % key] = np.asarray([N, M, size, seed, int(floats)], np.int64)
    out['%s/rotation' % key] = np.asarray(rotation, np.float64)
    if mean is not None:
        out['%s/mean' % key] = np.asarray(mean, np.float64)
        out['%s/std' % key] = np.asarray(std, np.float64)


def main():
    chaos = _load('ref_chaos_transform', 'datasetchaos_proposed')
    kidney = _load('ref_kidney_transform', 'datasetkidney_proposed')
    rng = np.random.RandomState(22)
    out = {}
    cases = []
    # u16 planes with values above 255 (PIL's I;16 -> RGB clamp), 256 x 256 source (identity resize), u8 views
    cases.append(('u16_256', chaos, True, [[block_plane(rng, 256, 256, 600), block_plane(rng, 256, 256, 400)]],
                  [mask_plane(rng, 256, 256)], 256, 60.0, 5, False, None, None))
    # down-sizing, square and non-square sources of different sizes in one batch, u8 views
    cases.append(('mixed_256', chaos, True, [[block_plane(rng, 288, 288), block_plane(rng, 288, 288)],
                                             [block_plane(rng, 200, 232), block_plane(rng, 200, 232)]],
                  [mask_plane(rng, 288, 288), mask_plane(rng, 200, 232)], 256, 60.0, 11, False, None, None))
    # the whole chain in float32: per-image Normalize, fixed data_mean / data_std, the single-modal (kidney) copy
    cases.append(('chaos_f32', chaos, True, [[smooth_plane(rng, 44, 40, noise=2), smooth_plane(rng, 44, 40, noise=2)],
                                             [smooth_plane(rng, 20, 24, noise=2), smooth_plane(rng, 20, 24, noise=2)]],
                  [mask_plane(rng, 44, 40), mask_plane(rng, 20, 24)], 32, 45.0, 17, True, None, None))
    cases.append(('fixed_f32', chaos, True, [[smooth_plane(rng, 44, 40, noise=2), smooth_plane(rng, 44, 40, noise=2)]],
                  [mask_plane(rng, 44, 40)], 32, 60.0, 23, True, [0.2, 0.25, 0.3], [0.3, 0.2, 0.25]))
    cases.append(('kidney_f32', kidney, False, [[smooth_plane(rng, 44, 40, noise=2)], [smooth_plane(rng, 36, 36, 300)]],
                  [mask_plane(rng, 44, 40), mask_plane(rng, 36, 36)], 32, 30.0, 29, True, None, None))
    for key, T, two, planes, masks, size, rot, seed, fl, mean, std in cases:
        run_case(out, key, T, two, planes, masks, size, rot, seed, fl, mean, std)
    out['cases'] = np.asarray([c[0] for c in cases])
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
