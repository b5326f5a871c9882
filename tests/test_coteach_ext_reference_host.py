"""CPU: makes the tables and the float64 references of tests/coteach_ext_cases.py binding.  Plain torch only: the tables reach
every path test_gpu_coteach_ext_paths.py is meant to reach (asserts, not skips), the operands hold the ties, ignored windows and
gaps the tables promise, the float64 references reproduce what the real reference recorded in the g7, g8, g17 (C = 3, 5) and g18
fixtures to the tolerances test_gpu_losses.py uses, they agree with the fp32 restatements in oracle/losses.py, and plain fp32 on
the CPU needs at most HALF the bound the GPU test uses on every case."""
import os

import numpy as np
import pytest
import torch

import oracle

import loss_cases as LC
import coteach_ext_cases as X

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
HALF = 0.5


# ------------------------------------------------------------------------------------------------- the tables
def test_ids_are_unique():
    for cases, name in ((X.MAP_CASES, X.map_id), (X.REGION_CASES, X.region_id), (X.SELECT_CASES, X.select_id)):
        assert len(set(cases)) == len(cases) and len(set(name(c) for c in cases)) == len(cases)
    assert X.MAP_MULTI_BLOCK in X.MAP_CASES and set(X.SATURATION_CASES) <= set(X.MAP_CASES)
    assert set(X.REGION_ABI_CASES) <= set(X.REGION_CASES)


def test_map_table_reaches_every_path():
    for g in X.MAP_SMALL:
        assert set(c.c for c in X.MAP_CASES if c[:3] == g) == set(range(2, 9)), g
    total = lambda c: c.n * c.h * c.w
    for two in (True, False):                       # the two-class kernels and the C-class templates, each ...
        mine = [c for c in X.MAP_CASES if (c.c == 2) == two]
        # ... past the grid cap with a ragged tail (`int grid1`: at most 4096 blocks of 256 threads)
        assert any(total(c) > X.GRID_CAP * X.BLOCK and total(c) % X.BLOCK for c in mine)
        # ... past the droppixel grid (aide_droppixel_*: at most 256 blocks of 256 threads per image) with a ragged tail
        assert any(c.h * c.w > X.DROPPIXEL_CAP * X.BLOCK and (c.h * c.w) % X.BLOCK for c in mine)
        assert any(c.h * c.w == 1 for c in mine) and any(1 < c.h * c.w < 64 for c in mine)
        assert any(1 < X.grid_blocks(total(c)) < X.GRID_CAP for c in mine)
    assert X.grid_blocks(total(X.MAP_MULTI_BLOCK)) > 1
    assert len([c for c in X.MAP_CASES if total(c) > 1 << 20]) == 2       # the large ones are single cases
    for c in X.MAP_CASES:                           # ndrop = 1 and N - 1, an unordered idx, an image left out
        splits = X.droppixel_splits(c.n)
        assert set(len(i) for i in splits) == {1, max(1, c.n - 1)}
        assert c.n < 3 or any(list(i) != sorted(i) for i in splits)
        assert all(len(set(i)) == len(i) and max(i) < c.n for i in splits)


def test_region_table_reaches_every_path():
    """region_win() and grid_blocks() restate `bool region_win` and `int grid1` of coteach_ext.hip"""
    win = lambda c: X.region_win(c.h, c.w, c.kh, c.kw)
    total = lambda c: X.region_count(c.n, c.h, c.w, c.kh, c.kw)
    for g in X.REGION_SMALL:
        assert set(c.c for c in X.REGION_CASES if c[:5] == g) == set(range(2, 9)), g
    for cc in X.CLASS_COUNTS:
        mine = [c for c in X.REGION_CASES if c.c == cc]
        assert any(not win(c) for c in mine) and any(win(c) for c in mine)
        assert any(win(c) and (c.kh, c.kw) == (2, 2) and c.h % 2 and c.w % 2 for c in mine)          # the 2x2 fallback
        for k in ((3, 3), (4, 4), (1, 3), (3, 1)):
            assert any((c.kh, c.kw) == k for c in mine), (cc, k)
        assert any(win(c) and c.h % c.kh and c.w % c.kw for c in mine)                               # clipped on both sides
    past = [c for c in X.REGION_CASES if total(c) > X.GRID_CAP * X.BLOCK]
    assert sorted((win(c), c.c) for c in past) == [(False, 2), (False, 3), (True, 2)] and past == list(X.REGION_LARGE)
    assert all(total(c) % X.BLOCK for c in past)
    assert any(1 < X.grid_blocks(total(c)) < X.GRID_CAP and win(c) for c in X.REGION_CASES)
    assert any(1 < X.grid_blocks(total(c)) < X.GRID_CAP and not win(c) for c in X.REGION_CASES)
    assert any(win(c) for c in X.REGION_ABI_CASES) and any(not win(c) and c.c == 2 for c in X.REGION_ABI_CASES) and \
        any(not win(c) and c.c > 2 for c in X.REGION_ABI_CASES)
    assert all(c.h * c.w < 1 << 31 for c in X.REGION_CASES)


def test_select_table_reaches_every_path():
    ms = sorted(set(c.m for c in X.SELECT_CASES))
    assert ms == [1, 35, 1023, 1024, 1025, 5000, 1026 * 1026]
    assert [X.cpt(m) for m in ms] == [1, 1, 1, 1, 2, 5, 1029]
    assert any(m < X.SELECT_THREADS for m in ms) and any(m > X.SELECT_THREADS for m in ms)
    for m in ms[:-1]:
        assert set((c.nseg, c.stride - c.m) for c in X.SELECT_CASES if c.m == m) == {(1, 0), (3, 0), (3, 24)}
    assert set((c.nseg, c.stride - c.m) for c in X.SELECT_CASES if c.m == ms[-1]) == {(1, 0), (1, 24)}


# ------------------------------------------------------------------------------------------------- the operands
def test_map_operands_are_as_the_table_says():
    for c in X.MAP_CASES:
        o = X.map_operands(c)
        assert o.z1.dtype == torch.float32 and o.z1.shape == o.z2.shape == (c.n, c.c, c.h, c.w) and o.t.shape == (c.n, c.h, c.w)
        assert (o.z3 is not None) == (c.c == 2)
        assert (c.w >= 5) == bool((o.t[0, 0, :5] == X.IGNORE).all()) == bool((o.t == c.c + 2).any())
        inside = o.t[(o.t != X.IGNORE) & (o.t != c.c + 2)]
        assert int(inside.min()) >= 0 and int(inside.max()) < c.c
    for c in X.SATURATION_CASES:
        o = X.saturated(c)
        for z in (o.z1, o.z2):
            d = z[:, 1] - z[:, 0]
            assert d.max().item() >= 80.0 and d.min().item() <= -80.0 and bool(torch.isfinite(z).all())


def test_region_operands_are_as_the_table_says():
    for c in X.REGION_CASES:
        z, t = X.region_operands(c)
        n, h, w, kh, kw, cc = c
        zp, tp = X.pooled(z.double(), t, kh, kw)
        assert zp.shape[2:] == (-(-h // kh), -(-w // kw)) == tp.shape[1:]
        if n == 1:
            continue
        win0 = t[0, :kh, :kw]
        assert int(tp[0, 0, 0]) == X.IGNORE and bool((win0 == X.IGNORE).any())
        assert kh * kw == 1 or bool((win0 != X.IGNORE).any())                      # an ignored pixel among labelled ones
        for k in range(cc):
            patch = z[0, k, :kh, kw:2 * kw]
            assert bool((patch == patch[0, 0]).all())                                # every position ties
            two = z[0, k, kh:2 * kh, :kw]
            assert two[0, 0] == two.max() and two[-1, -1] == two.max() and (kh * kw == 1 or (two == two.max()).sum() == 2)
        assert bool((t[2] == X.IGNORE).all()) and bool((tp[2] == X.IGNORE).all())
        assert X.out_of_class_window(c) == (int(tp[1, 0, 0]) == cc + 1)
        cls = X.region_class(tp, cc, X.region_win(h, w, kh, kw))
        assert int(cls[cls != X.IGNORE].max()) < cc and bool((cls[1:2] != X.IGNORE).any())
        # the float64 gradient goes to the first maximum of a tied window and nowhere else in it
        v, mask, dz = X.region_reference(c)
        for i, (r0, c0) in ((1, (0, kw)), (-(-w // kw), (kh, 0))):
            assert mask[0, i] == 1 and v[0, i] > 0
            blk = dz[0, :, r0:r0 + kh, c0:c0 + kw]
            assert bool((blk[:, 0, 0] != 0).all()) and int((blk != 0).sum()) == cc
        assert mask[1, 0] == 1 and mask[0, 0] + mask[2].sum() > 0      # masked, ignored regions: the backward must leave 0
        if X.out_of_class_window(c):                                    # no class: no loss, and not a single gradient word
            assert v[1, 0] == 0 and not bool(dz[1, :, :kh, :kw].any())
    assert any(X.out_of_class_window(c) for c in X.REGION_CASES if c.c == 3)
    assert not any(X.out_of_class_window(c) for c in X.REGION_CASES if c.c == 2)


@pytest.mark.parametrize('case', X.SELECT_CASES, ids=X.select_id)
def test_select_operands_and_reference(case):
    """the values hold what the table says, and the reference is numpy's stable argsort"""
    sel, sums = X.select_values(case)
    m, nseg, stride = case
    assert sel.shape == sums.shape == (nseg, stride) and bool(torch.isnan(sel[:, m:]).all())
    assert bool(torch.isfinite(sums).all()) and float(sums.min()) >= 0.5
    a, length = X.tie_run(m)
    assert length > X.cpt(m) or length == m
    assert a // X.cpt(m) != (a + length - 1) // X.cpt(m) or m == 1                  # the run crosses thread ranges
    for s in range(0, nseg, 2):
        v = sel[s, :m]
        assert bool((v[a:a + length] == X.TIE).all())
        if m >= 35:
            bits = v[:10].view(torch.int32).tolist()
            assert bits[0] == 0 and bits[1] == -2 ** 31 and bits[8] == -2 ** 31 and bits[9] == 0          # both zeros
            assert 0 < abs(float(v[2])) < 1.2e-38 and float(v[3]) == -float(v[2])                         # denormals
            assert float(v[4]) == float('inf') and bits[5] > 0 and bits[6] < 0 and bool(torch.isnan(v[5:7]).all())
            assert bool((v < 0).any())
    if nseg > 1:
        assert bool((sel[1, :m] == sel[1, 0]).all())
    for only_positive in (False, True):
        forms = X.select_ks(case, only_positive)
        cand = X.candidates(sel[0, :m], only_positive)
        count = int(cand.sum())
        below = int((cand & (sel[0, :m] < X.TIE)).sum())
        ks = [k for k, rr, kin in forms if rr < 0 and kin is None]
        assert 0 in ks and count in ks and count + 5 in ks and (m == 1 or 1 in ks)
        assert any(below < k < below + length for k in ks) or length == 1           # a cut inside the tie run
        assert any(rr >= 0 and rr * count != int(rr * count) for _, rr, _ in forms) or count <= 1
        assert any(kin is not None for _, _, kin in forms)
        for k_host, rr, k_in in forms:
            mask, tot, kk = X.select_reference(case, k_host, rr, k_in, only_positive)
            for s in range(nseg):
                v = sel[s, :m].numpy()
                c = (v > 0) if only_positive else np.ones(m, bool)
                idx = np.nonzero(c)[0]
                order = idx[np.argsort(v[idx], kind='stable')]
                ref = np.zeros(m, np.uint8)
                ref[order[:int(kk[s])]] = 1
                assert int(kk[s]) == X.select_k(len(idx), k_host, rr, k_in) and (ref == mask[s].numpy()).all()
                assert int(mask[s].sum()) == int(kk[s])


@pytest.mark.parametrize('c', X.MODULE_CLASSES)
def test_module_operands_obey_the_gap_rule(c):
    z1, z2, t = X.region_module_operands(c)
    assert X.region_module_gap(z1, z2, t) > X.SEL_GAP
    kinds = set(X.region_win(z1.shape[2], z1.shape[3], *X.region_windows(z1.shape[2], z1.shape[3], s)) for s in X.REGION_SCALES)
    assert kinds == {True, False}
    assert [X.region_windows(46, 50, s) for s in X.REGION_SCALES] == [(2, 2), (3, 3), (4, 4), (1, 1)]
    z1, z2, z3, t = X.pixel_module_operands(c)
    assert X.pixel_module_gap(z1, z2, z3, t) > X.SEL_GAP
    o = LC.coteach_operands(z1.shape[0], c)._replace(z1=z1, z2=z2, t1=t, t2=t)
    assert LC.coteach_min_gap(o) > LC.MIN_GAP
    assert (c == 2) != bool((t == X.IGNORE).any())
    # every forget rate cuts somewhere else: none kept, some, all
    assert [X.droppixel_keep(fr, 3) for fr in X.FORGET_RATES] == [3, 2, 1, 0]


# ------------------------------------------------------------------------------------------------- against the recorded values
def _close(got, want, what, rtol=1e-4):
    """`close` of test_gpu_losses.py"""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(np.asarray(want)).double()
    err = (got - want).abs().max().item()
    assert err <= rtol * (want.abs().max().item() + 1e-12) + 1e-9, '%s: err %.3e' % (what, err)


def _mostly(got, want, what):
    """the gradient comparison of test_coteach_ext_g7: the recorded fp32 selection may differ from the float64 one between values
    closer than fp32 noise"""
    got, want = got.numpy(), np.asarray(want, dtype=np.float64)
    bad = np.abs(got - want) > 1e-4 * max(np.abs(want).max(), 1e-30) + 1e-12
    assert bad.mean() < 2e-4, (what, int(bad.sum()))


def _kl_fixture(z1, z2, fx, pre, rtol):
    a, b = z1.double().requires_grad_(True), z2.double().requires_grad_(True)
    v = X.kl_map(a, b)
    (v * torch.linspace(0.5, 1.5, v.numel()).view_as(v)).sum().backward()
    _close(v.detach(), fx[pre + 'KL/map'], 'KL map', rtol)
    _close(a.grad, fx[pre + 'KL/grad1'], 'KL grad1', rtol)
    _close(b.grad, fx[pre + 'KL/grad2'], 'KL grad2', rtol)


def _ext_fixture(z1, z2, t, fx, pre, rates):
    for fr in rates:
        r = X.region_module_reference(z1, z2, t, 0.5, fr)
        key = '%sCoteachingloss_dropregionce/fr%g' % (pre, fr)
        zero = torch.zeros_like(r['grad1'])
        for which, grads in ((1, (r['grad1'], zero)), (2, (zero, r['grad2']))):
            assert abs(r['loss%d' % which].item() - float(fx[key + '/loss%d' % which])) < 1e-5 * abs(float(fx[key + '/loss%d' % which]))
            for k, g in enumerate(grads):
                _mostly(g, fx[key + '/l%d_grad%d' % (which, k + 1)], key)
        r = X.droppixel_module_reference(z1, z2, t, fr)
        key = '%sCoteachingloss_dropimagedroppixel/fr%g' % (pre, fr)
        for which in (1, 2):
            assert abs(r['loss%d' % which].item() - float(fx[key + '/loss%d' % which])) < 1e-5 * abs(float(fx[key + '/loss%d' % which]))
            for k in (1, 2):
                _mostly(r['l%d_grad%d' % (which, k)], fx[key + '/l%d_grad%d' % (which, k)], key)


def test_reference_reproduces_g7():
    g3, fx = np.load(os.path.join(GOLD, 'g3_losses.npz')), np.load(os.path.join(GOLD, 'g7_coteach_ext.npz'))
    z1, z2, t = (torch.from_numpy(g3[k]) for k in ('z1', 'z2', 'targets'))
    _kl_fixture(z1, z2, fx, '', 2e-5)
    _ext_fixture(z1, z2, t, fx, '', (0.0, 0.25, 0.5))


@pytest.mark.parametrize('C', [3, 5])
def test_reference_reproduces_g17(C):
    fx, pre = np.load(os.path.join(GOLD, 'g17_multiclass.npz')), 'c%d/' % C
    z1, z2, t = (torch.from_numpy(fx[pre + k]) for k in ('z1', 'z2', 'targets'))
    _kl_fixture(z1, z2, fx, pre, 2e-5)
    _ext_fixture(z1, z2, t, fx, pre, (0.25, 0.5))


def test_reference_reproduces_g18():
    g3, fx = np.load(os.path.join(GOLD, 'g3_losses.npz')), np.load(os.path.join(GOLD, 'g18_dropregionce_scale.npz'))
    cases = {'c2': tuple(torch.from_numpy(g3[k]) for k in ('z1', 'z2', 'targets')),
             'c3': tuple(torch.from_numpy(fx['c3/' + k]) for k in ('z1', 'z2', 'targets'))}
    for cname, (z1, z2, t) in cases.items():
        for scale in (0.25, 0.3):
            for fr in (0.25, 0.5):
                key = '%s/s%g/fr%g' % (cname, scale, fr)
                r = X.region_module_reference(z1, z2, t, scale, fr)
                for which in (1, 2):
                    ref = float(fx[key + '/loss%d' % which])
                    assert abs(r['loss%d' % which].item() - ref) < 1e-5 * abs(ref), key
                    _mostly(r['grad%d' % which], fx[key + '/grad%d' % which], key)


def test_reference_reproduces_g8():
    g3, fx = np.load(os.path.join(GOLD, 'g3_losses.npz')), np.load(os.path.join(GOLD, 'g8_pixelcoreg.npz'))
    z1, z2, t = (torch.from_numpy(g3[k]) for k in ('z1', 'z2', 'targets'))
    for cname, z3 in (('Pixelcoreg_Focalloss', torch.from_numpy(fx['z3'])), ('Pixelcoreg_Focalloss_twomodel', None)):
        for fr, kd, red in ((0.0, 0.3, 'mean'), (0.25, 0.3, 'mean'), (0.5, 0.7, 'sum')):
            key = '%s/fr%g_kd%g_%s' % (cname, fr, kd, red)
            r = X.pixelcoreg_module_reference(z1, z2, z3, t, fr, kd, red)
            assert abs(r['loss'].item() - float(fx[key + '/loss'])) < 2e-5 * abs(float(fx[key + '/loss'])), key
            assert abs(r['frac'].item() - float(fx[key + '/frac'])) < 2e-3
            grads = [torch.zeros_like(r['grads'][0])] * 2 + r['grads'] if z3 is not None else r['grads']
            for i, g in enumerate(grads):
                _mostly(g, fx[key + '/grad%d' % (i + 1)], key)


# ------------------------------------------------------------------------------------------------- against the fp32 oracle
@pytest.mark.parametrize('c', X.MODULE_CLASSES)
def test_reference_agrees_with_the_oracle(c):
    """the fp32 restatements of the reference in oracle/losses.py on the module operands: the gap rule makes their selections
    the float64 ones, values and gradients agree within half the bound"""
    worst = [(0.0, '')]

    def close(got, ref, what):
        e = LC.rel_err(got, ref)
        worst[0] = max(worst[0], (e, what))
        assert e <= HALF, (what, e)

    z1, z2, t = X.region_module_operands(c)
    for scale in X.REGION_SCALES:
        for fr in X.FORGET_RATES:
            a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
            l1, l2 = oracle.Coteachingloss_dropregionce(scale=scale, reduction='none')(a, b, t, fr)
            (l1 + l2).backward()
            r = X.region_module_reference(z1, z2, t, scale, fr)
            for got, k in ((l1, 'loss1'), (l2, 'loss2'), (a.grad, 'grad1'), (b.grad, 'grad2')):
                close(got, r[k], 'dropregionce s=%g fr=%g %s' % (scale, fr, k))
    z1, z2, z3, t = X.pixel_module_operands(c)
    close(oracle.KLbidirection(z1, z2), X.kl_map(z1.double(), z2.double()), 'KLbidirection')
    for fr in X.FORGET_RATES[:-1]:            # at 1.0 the oracle indexes an empty keep set of images
        r = X.droppixel_module_reference(z1, z2, t, fr, 0.7)
        for which in (1, 2):
            a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
            ls = oracle.Coteachingloss_dropimagedroppixel(weight=0.7, reduction='none')(a, b, t, fr)
            ls[which - 1].backward()
            close(ls[which - 1], r['loss%d' % which], 'droppixel fr=%g loss%d' % (fr, which))
            for k, x in ((1, a), (2, b)):
                g = torch.zeros_like(z1) if x.grad is None else x.grad
                close(g, r['l%d_grad%d' % (which, k)], 'droppixel fr=%g l%d_grad%d' % (fr, which, k))
    if c == 2:
        for three in (True, False):
            for fr, kd, red in ((0.0, 0.3, 'mean'), (0.25, 0.3, 'mean'), (0.5, 0.7, 'sum'), (1.0, 0.3, 'sum')):
                zs = [z.clone().requires_grad_(True) for z in ((z1, z2, z3) if three else (z1, z2))]
                op = oracle.Pixelcoreg_Focalloss if three else oracle.Pixelcoreg_Focalloss_twomodel
                loss, frac = op(reduction=red)(*zs, t, fr, kd)
                r = X.pixelcoreg_module_reference(z1, z2, z3 if three else None, t, fr, kd, red)
                what = 'pixelcoreg three=%d fr=%g' % (three, fr)
                close(loss, r['loss'], what)
                close(torch.as_tensor(frac), r['frac'], what + ' frac')
                if fr < 1.0:
                    loss.backward()
                    for x, g in zip(zs[2:] if three else zs, r['grads']):
                        close(x.grad, g, what + ' grad')
    print('C=%d worst fp32 oracle error %.3f of the GPU bound (%s)' % ((c,) + worst[0]))


# ------------------------------------------------------------------------------------------------- plain fp32 has room
def _fp32(fn, inputs, mask, coeff=X.COEFF):
    return X.masked_backward(fn, inputs, mask, coeff, torch.float32)


@pytest.mark.parametrize('case', X.MAP_CASES, ids=X.map_id)
def test_fp32_maps_within_half_the_bound(case):
    o = X.map_operands(case)
    worst = (0.0, '')
    v, gout, g1, g2 = X.kl_reference(case)
    fv, fg = _fp32(X.kl_map, (o.z1, o.z2), gout, 1.0)
    worst = max(worst, (LC.rel_err(fv, v), 'kl'), (LC.rel_err(fg[0], g1), 'kl g1'), (LC.rel_err(fg[1], g2), 'kl g2'))
    if case.n * case.h * case.w < 1 << 20:
        for idx in X.droppixel_splits(case.n):
            for which in (0, 1):
                v, mask, g1, g2 = X.droppixel_reference(case, idx, which)
                fv, fg = _fp32(lambda a, b: X.droppixel_map(a, b, o.t, idx, which), (o.z1, o.z2), mask)
                worst = max(worst, (LC.rel_err(fv, v), 'droppixel'), (LC.rel_err(fg[0], g1), 'droppixel g1'),
                            (LC.rel_err(fg[1], g2), 'droppixel g2'))
    if case.c == 2:
        key, val, tf, mask, grads = X.pixelcoreg_reference(case, False)
        fv, fg = _fp32(lambda a, b: X.pixelcoreg_maps(a, b, None, o.t, 0.3)[0], (o.z1, o.z2), mask)
        worst = max(worst, (LC.rel_err(fv, key), 'coreg key'), (LC.rel_err(fg[0], grads[0]), 'coreg g1'),
                    (LC.rel_err(fg[1], grads[1]), 'coreg g2'))
        key, val, tf, mask, grads = X.pixelcoreg_reference(case, True)
        fv, fg = _fp32(lambda c3: X.pixelcoreg_maps(o.z1, o.z2, c3, o.t, 0.3)[1], (o.z3,), mask)
        worst = max(worst, (LC.rel_err(fv, val), 'coreg val'), (LC.rel_err(fg[0], grads[0]), 'coreg g3'))
    print('%-18s worst fp32 error %.3f of the GPU bound (%s)' % ((X.map_id(case),) + worst))
    assert worst[0] <= HALF, worst


@pytest.mark.parametrize('case', X.REGION_CASES, ids=X.region_id)
def test_fp32_region_ce_within_half_the_bound(case):
    z, t = X.region_operands(case)
    v, mask, dz = X.region_reference(case)
    fv, (fdz,) = _fp32(lambda a: X.region_ce(a, t, case.kh, case.kw), (z,), mask)
    assert torch.equal(fdz == 0, dz == 0)                    # fp32 max-pooling routes to the same positions
    worst = max((LC.rel_err(fv, v), 'loss'), (LC.rel_err(fdz, dz), 'dz'))
    print('%-24s worst fp32 error %.3f of the GPU bound (%s)' % ((X.region_id(case),) + worst))
    assert worst[0] <= HALF, worst


@pytest.mark.parametrize('case', X.SATURATION_CASES, ids=X.map_id)
def test_fp32_on_saturated_logits(case):
    o = X.saturated(case)
    mask = torch.ones(o.t.shape, dtype=torch.uint8)
    v, g = X.masked_backward(X.kl_map, (o.z1, o.z2), mask)
    fv, fg = _fp32(X.kl_map, (o.z1, o.z2), mask)
    assert bool(torch.isfinite(v).all()) and all(bool(torch.isfinite(x).all()) for x in g)
    assert LC.rel_err(fv, v) <= HALF and LC.rel_err(fg[0], g[0]) <= HALF and LC.rel_err(fg[1], g[1]) <= HALF
