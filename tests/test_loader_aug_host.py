"""CPU: the loader-transform entry points (aide_amd/csrc/augment.hip, utils/loader_aug.py) -- symbols, argument checks
without a device, the random draws against fixture g22 (the reference's transform.py run under a seeded `random`), and
the host tables (PIL's resampling coefficients, its NEAREST index rule) against PIL itself."""
import os
import random
import subprocess

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAMES = ('aide_loader_aug', 'aide_loader_aug_ws_bytes', 'aide_loader_mask_onehot')


@pytest.fixture(scope='module')
def built():
    from aide_amd.build import build
    return build(verbose=False)


def test_loader_aug_symbols(built):
    from aide_amd._lib import parse_header
    protos = parse_header()
    out = subprocess.run(['nm', '-D', '--defined-only', built], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for n in NAMES:
        assert n in protos and n in exported, n
    from aide_amd import utils as U
    assert U.LoaderAugment and U.draw_aug_params and U.CHAOS_PALETTE == (0, 63, 126, 189, 252)


def test_loader_aug_bad_arguments(built):
    from aide_amd._lib import lib
    ERR = -1
    p = 16      # any non-NULL address: every call below is refused before a launch
    args = dict(src=p, desc=p, tab=p, par=p, norm=None, N=2, M=2, S=8, augno=4, out_u8=0, out=p, ws=p)

    def call(**kw):
        a = dict(args, **kw)
        return lib.aide_loader_aug(a['src'], a['desc'], a['tab'], a['par'], a['norm'], a['N'], a['M'], a['S'], a['augno'],
                                   a['out_u8'], a['out'], a['ws'], None)
    for k in ('src', 'desc', 'tab', 'out', 'ws', 'par'):
        assert call(**{k: None}) == ERR, k
    for k in ('N', 'M', 'S'):
        assert call(**{k: 0}) == ERR and call(**{k: -3}) == ERR, k
    assert call(augno=5) == ERR and call(augno=-1) == ERR
    assert call(ws=p + 4) == ERR          # workspace alignment
    assert lib.aide_loader_aug_ws_bytes(0, 8) == 0 and lib.aide_loader_aug_ws_bytes(2, 0) == 0
    assert lib.aide_loader_aug_ws_bytes(4, 256) >= 4 * 256 * 256
    m = lib.aide_loader_mask_onehot
    assert m(None, p, p, p, 2, 8, 5, p, None) == ERR and m(p, p, p, None, 2, 8, 5, p, None) == ERR
    assert m(p, p, p, p, 2, 8, 5, None, None) == ERR
    assert m(p, p, p, p, 2, 8, 9, p, None) == ERR and m(p, p, p, p, 2, 8, 0, p, None) == ERR
    assert m(p, p, p, p, 0, 8, 5, p, None) == ERR and m(p, p, p, p, 2, -1, 5, p, None) == ERR


def test_draw_aug_params_matches_reference_g22():
    from aide_amd.utils.loader_aug import draw_aug_params
    fx = np.load(os.path.join(GOLD, 'g22_loader_aug.npz'))
    for key in fx['cases']:
        n, _, _, seed, _ = fx['%s/meta' % key]
        d = draw_aug_params(int(n), float(fx['%s/rotation' % key]), random.Random(int(seed)))
        assert d['augno'] == [4] * int(n)
        for k in range(4):
            assert d['degree%d' % (k + 1)] == fx['%s/degree' % key][k].tolist(), key      # exact
            assert d['hflip%d' % (k + 1)] == fx['%s/hflip' % key][k].tolist(), key


def test_resize_tables_match_pil():
    """the bilinear coefficient tables (through the numpy model of the device resize) and the NEAREST index tables equal
    PIL on a size sweep: up, down, identity, odd, non-square, u16 clamp"""
    from PIL import Image
    from aide_amd.utils.loader_aug import resize_bilinear_model, nearest_index
    rng = np.random.RandomState(3)
    for h, w, s in ((288, 288, 256), (200, 232, 256), (72, 80, 64), (7, 9, 5), (3, 3, 64), (100, 37, 256), (640, 480, 256),
                    (2, 3, 3), (33, 17, 40), (256, 256, 256), (1, 1, 4), (255, 257, 256)):
        a = rng.randint(0, 256, (h, w)).astype(np.uint8)
        ref = np.array(Image.fromarray(a).convert('RGB').resize((s, s), Image.BILINEAR))[:, :, 0]
        assert np.array_equal(resize_bilinear_model(a, s), ref), (h, w, s)
        m = rng.randint(0, 256, (h, w)).astype(np.uint8)
        refm = np.array(Image.fromarray(m).resize((s, s), Image.NEAREST))
        assert np.array_equal(m[nearest_index(h, s)][:, nearest_index(w, s)], refm), (h, w, s)
    u = rng.randint(0, 1000, (30, 34)).astype(np.uint16)
    ref = np.array(Image.fromarray(u).convert('RGB').resize((24, 24), Image.BILINEAR))[:, :, 0]
    assert np.array_equal(resize_bilinear_model(u, 24), ref)
    bad = 0
    for i in range(1, 70):
        for o in range(1, 70):
            col = np.arange(i, dtype=np.uint8)[None, :]
            bad += not np.array_equal(np.array(Image.fromarray(col).resize((o, 1), Image.NEAREST))[0], nearest_index(i, o))
    assert bad == 0


def _onehot_ref(m, palette):
    """PIL NEAREST-resized mask -> dataset.py's one_hot_mask layout [len(palette), S, S]"""
    return np.stack([(m == c).astype(np.int64) for c in palette])


def test_pack_rows_point_at_their_planes():
    """every descriptor row of the packed upload points at the bytes, height and width of its own plane -- source rows
    p = n * M + m, mask rows q * N + n -- with several masks per sample of different sizes; and the mask rows decoded
    through their NEAREST tables equal PIL + one_hot_mask"""
    from PIL import Image
    from aide_amd.utils.loader_aug import LoaderAugment, draw_aug_params, CHAOS_PALETTE
    rng = np.random.RandomState(8)
    S, N, M, Q = 24, 3, 2, 3
    imgs = [tuple(rng.randint(0, 256, (20 + 3 * n + m, 22 + n)).astype(np.uint8) for m in range(M)) for n in range(N)]
    pal = np.asarray(CHAOS_PALETTE + (100,), np.uint8)
    masks = [tuple(pal[rng.randint(0, 6, (16 + 5 * q + 2 * n, 30 - 4 * q + n))] for q in range(Q)) for n in range(N)]
    aug = LoaderAugment(S, 60.0)
    pk, o = aug.pack(imgs, draw_aug_params(N, 60.0, random.Random(1)), masks=masks)
    buf = pk.host()
    desc = buf[o['desc']:o['desc'] + N * M * 32].view(np.int32).reshape(N * M, 8)
    for n in range(N):
        for m in range(M):
            off, h, w = desc[n * M + m, :3]
            a = imgs[n][m]
            assert (h, w) == a.shape and np.array_equal(buf[off:off + h * w].reshape(h, w), a), (n, m)
    assert o['Q'] == Q
    mdesc = buf[o['mdesc']:o['mdesc'] + Q * N * 32].view(np.int32).reshape(Q * N, 8)
    tab = buf[o['tab']:].view(np.int32)
    for q in range(Q):
        for n in range(N):
            off, h, w, _, xo, yo = mdesc[q * N + n, :6]
            a = masks[n][q]
            plane = buf[off:off + h * w].reshape(h, w)
            assert (h, w) == a.shape and np.array_equal(plane, a), (q, n)
            got = _onehot_ref(plane[tab[yo:yo + S]][:, tab[xo:xo + S]], CHAOS_PALETTE)
            ref = _onehot_ref(np.array(Image.fromarray(a).resize((S, S), Image.NEAREST)), CHAOS_PALETTE)
            assert np.array_equal(got, ref), (q, n)
