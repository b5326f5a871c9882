"""CPU: makes the table and the float64 reference of tests/loss_cases.py binding.  Host-side queries of the library only
(aide_seg_loss_blocks) and plain torch: the table reaches every block split test_gpu_loss_paths.py is meant to reach (an
assert, not a skip); the float64 reference reproduces the values and gradients the real reference recorded in the g3, g12 and
g17 fixtures (C = 2, 3, 5, 8) within their fp32 noise; on every table case the fp32 oracle agrees with the float64 reference
within HALF the bound the GPU test uses, so a kernel in plain fp32 has room; and the conditions under which the GPU test
compares integers exactly (argsort, hard statistics, labels) hold for the inputs of every case."""
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import steps

import loss_cases as LC
from multiclass_cases import loss_cases as g17_forms, targets_of

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
IDS = [LC.case_id(c) for c in LC.CASES]
HALF = 0.5                      # of the GPU bound (LC.rel_err counts in units of 1e-4 max |ref| + 1e-9)


@pytest.fixture(scope='module')
def L():
    from aide_amd.build import build
    build(verbose=False)
    from aide_amd._lib import lib
    return lib.load()            # raw entry points: host-state queries


def test_table_is_well_formed():
    assert len(set(LC.CASES)) == len(LC.CASES) and len(set(IDS)) == len(IDS)
    for n, h, w in LC.GEOMETRIES:
        assert set(c.c for c in LC.CASES if (c.n, c.h, c.w) == (n, h, w)) == set(range(2, 9)), (n, h, w)
    assert set(c.c for c in LC.CASES if (c.n, c.h, c.w) == LC.BATCH_GEOMETRY) == {2, 5}
    assert set(LC.ABI_CASES) <= set(LC.CASES) and set(LC.SATURATION_CASES) <= set(LC.CASES)
    assert set(c.c for c in LC.ABI_CASES) == set(LC.COTEACH_CLASSES) == {2, 4, 7}
    assert any(c.n == 1 for c in LC.CASES) and any(c.n > 256 for c in LC.CASES)


def test_table_reaches_every_block_split(L):
    """blocks per image as the library itself cuts HW: 1, 2, 3 and the 64-block cap with more than one stride per thread,
    each at every class count"""
    need = {'bpi 1': lambda bpi, hw: bpi == 1, 'bpi 2': lambda bpi, hw: bpi == 2, 'bpi 3': lambda bpi, hw: bpi == 3,
            'bpi 64, capped': lambda bpi, hw: bpi == 64 and hw > 64 * 256}
    for what, hit in need.items():
        for cc in LC.CLASS_COUNTS:
            assert any(hit(L.aide_seg_loss_blocks(c.h * c.w), c.h * c.w) for c in LC.CASES if c.c == cc), (what, cc)
    for c in LC.ABI_CASES:
        assert L.aide_seg_loss_blocks(c.h * c.w) in (2, 3)
    assert L.aide_seg_loss_blocks(LC.COTEACH_HW[0] * LC.COTEACH_HW[1]) == 2
    # every multi-block case ends in a partial stride
    for c in LC.CASES:
        assert L.aide_seg_loss_blocks(c.h * c.w) == 1 or (c.h * c.w) % 256 != 0, c


def test_operands_are_as_the_table_says():
    for c in LC.CASES:
        o = LC.operands(c)
        assert o.z.dtype == torch.float32 and o.z.shape == (c.n, c.c, c.h, c.w) and o.t.shape == (c.n, c.h, c.w)
        valid = o.t != LC.IGNORE
        assert int(o.t[valid].min()) >= 0 and int(o.t[valid].max()) < c.c
        assert (c.w >= 5) == bool((o.t[0, 0, :5] == LC.IGNORE).all())
        assert len(o.class_w) == c.c and o.class_w[0] == 0.5 and o.class_w[-1] == 2.0
        assert torch.allclose(o.pseudo.sum(1), torch.ones(c.n, c.h, c.w), atol=1e-6)
        assert torch.equal(o.wmap[:, 0], 1.0 - 4.0 * o.pseudo[:, 0] * o.pseudo[:, 1])
        if (c.n, c.h, c.w) == LC.EDGE_GEOMETRY:
            assert not o.t[1].any() and bool((o.t[2] == LC.IGNORE).all())
    for c in LC.SATURATION_CASES:
        z = LC.saturated(c)
        d = z[:, 1] - z[:, 0]
        assert d.max().item() >= 80.0 and d.min().item() <= -80.0 and bool(torch.isfinite(z).all())


# ------------------------------------------------------------------------------- the reference against the real reference
def _fixture_close(got, want, what):
    """the bound the fixture tests use: 1e-4 of scale"""
    assert LC.rel_err(got, torch.from_numpy(np.asarray(want))) <= 1.0, what


def _ones(v):
    return torch.ones_like(v)


def test_reference_reproduces_g3():
    fx = np.load(os.path.join(GOLD, 'g3_losses.npz'))
    z1, z2, t = torch.from_numpy(fx['z1']), torch.from_numpy(fx['z2']), torch.from_numpy(fx['targets'])
    for wname, cw, cdw in (('w11', [1.0, 1.0], [1.0, 1.0]), ('w13', [1.0, 3.0], [0.7, 1.6])):
        for lname, kw in (('CrossEntropyLoss2d', dict(weight=cw)), ('MulticlassDiceLoss', dict(weight=cw)), ('DiceLoss', {}),
                          ('CEMDiceLoss', dict(cediceweight=cdw, ceclassweight=cw, diceclassweight=cw)),
                          ('CEMDiceLossImage', dict(cediceweight=cdw, ceclassweight=cw, diceclassweight=cw))):
            v, g = LC.module_reference(lname, kw, z1, t, up=_ones)
            _fixture_close(v, fx['%s/%s' % (lname, wname)], lname + wname)
            _fixture_close(g, fx['%s/%s/grad' % (lname, wname)], lname + wname + ' grad')
    for red in ('none', 'sum'):
        v, _ = LC.module_reference('CrossEntropyLoss2d', dict(weight=[1.0, 3.0], reduction=red), z1, t)
        _fixture_close(v, fx['CrossEntropyLoss2d/w13/' + red], 'CE ' + red)
    _fixture_close(LC.hard_dice_sum(LC.statistics(z1.double(), t)), fx['Dice_fn'], 'Dice_fn')
    v, g = LC.module_reference('MulticlassMSELoss', dict(reduction='none'), z1, torch.from_numpy(fx['pseudo']),
                               weight_map=torch.from_numpy(fx['wmap']))
    _fixture_close(v, fx['mse_wm_mean'], 'mse')
    _fixture_close(g, fx['mse_wm_mean/grad'], 'mse grad')
    # the two co-teaching operators: w_ce = weight = 1, w_dice = 1, keep = int((1 - forget rate) N)
    for variant, cname in ((1, 'Coteachingloss_dropimage'), (2, 'Coteachingloss_weightimage')):
        for fr in (0.0, 0.25, 0.5):
            r = LC.coteach_reference(z1, z2, t, t, variant, int((1 - fr) * z1.shape[0]), 1.0, 1.0)
            key = '%s/fr%g' % (cname, fr)
            for k in ('loss1', 'loss2', 'grad1', 'grad2'):
                _fixture_close(r[k], fx['%s/%s' % (key, k)], key + k)
            assert r['argsort1'].tolist() == fx['coteach/argsort1'].tolist()
            assert r['argsort2'].tolist() == fx['coteach/argsort2'].tolist()
            _fixture_close(r['per_image1'], fx['coteach/per_image1'], 'per image')


def test_reference_reproduces_g12():
    from test_gpu_losses import G12_LOSSES, G12_BATCHES, G12_BRANCHES
    fx = np.load(os.path.join(GOLD, 'g12_metrics.npz'))
    z, t = torch.from_numpy(fx['z']), torch.from_numpy(fx['targets'])
    for batch, tag in G12_BATCHES:          # images that are empty in the target (and in the prediction): the T == 0 rule
        _fixture_close(LC.hard_dice_sum(LC.statistics(z[batch].double(), t[batch])), fx[tag + '/Dice_fn'], 'Dice_fn ' + tag)
    for lname, kw, key in G12_LOSSES:
        v, g = LC.module_reference(lname, kw, z, t, up=_ones)
        _fixture_close(v, fx[key], key)
        _fixture_close(g, fx[key + '/grad'], key + ' grad')
    onehot = torch.from_numpy(fx['onehot'])
    tgt = dict(onehot=onehot, t=t, onehot1=onehot[:, 1])
    ramp = lambda v: torch.arange(1, v.numel() + 1, dtype=v.dtype)
    for lname, kw, xin, tin, tag in G12_BRANCHES:
        key = 'branch/%s/%s/%s' % (lname, tin, tag)
        if xin == 'prob':
            v, g = LC.prob_dice_reference(torch.from_numpy(fx['prob']), tgt[tin], kw, up=ramp)
        else:
            v, g = LC.module_reference(lname, kw, z, tgt[tin], up=ramp)
        _fixture_close(v, fx[key], key)
        _fixture_close(g, fx[key + '/grad'], key + ' grad')


@pytest.mark.parametrize('C', [3, 5, 8])
def test_reference_reproduces_g17(C):
    fx, pre = np.load(os.path.join(GOLD, 'g17_multiclass.npz')), 'c%d/' % C
    z1, z2 = torch.from_numpy(fx[pre + 'z1']), torch.from_numpy(fx[pre + 'z2'])
    t = torch.from_numpy(fx[pre + 'targets'])
    for key, lname, kw, kind in g17_forms(fx, pre):
        v, g = LC.module_reference(lname, kw, z1, targets_of(fx, pre, kind, C))
        _fixture_close(v, fx[pre + key], key)
        _fixture_close(g, fx[pre + key + '/grad'], key + ' grad')
    _fixture_close(LC.hard_dice_sum(LC.statistics(z1.double(), t)), fx[pre + 'Dice_fn'], 'Dice_fn')
    pseudo, wmap = torch.from_numpy(fx[pre + 'pseudo']), torch.from_numpy(fx[pre + 'wmap'])
    v, g = LC.module_reference('MulticlassMSELoss', dict(reduction='none'), z1, pseudo, weight_map=wmap)
    _fixture_close(v, fx[pre + 'mse_wm_mean'], 'mse')
    _fixture_close(g, fx[pre + 'mse_wm_mean/grad'], 'mse grad')
    for variant, cname in ((1, 'Coteachingloss_dropimage'), (2, 'Coteachingloss_weightimage')):
        for fr in (0.25, 0.5):
            r = LC.coteach_reference(z1, z2, t, t, variant, int((1 - fr) * z1.shape[0]), 1.0, 1.0)
            for k in ('loss1', 'loss2', 'grad1', 'grad2'):
                _fixture_close(r[k], fx['%s%s/fr%g/%s' % (pre, cname, fr, k)], cname + k)
    # the proposed inline step: cross-scored selection, keep 2 of 4, consistency term on the dropped images
    r = LC.coteach_reference(z1, z2, t, t, 0, 2, float(fx[pre + 'cedice_w'][0]), float(fx[pre + 'cedice_w'][1]),
                             class_w=fx[pre + 'class_w'].tolist(), rate=0.3, w_seg=1.0, w_cor=10.0,
                             q1=pseudo, wm1=wmap, q2=pseudo, wm2=wmap)
    assert r['argsort1'].tolist() == fx[pre + 'proposed/indx1'].tolist()
    assert r['argsort2'].tolist() == fx[pre + 'proposed/indx2'].tolist()
    for k in ('loss1', 'loss2', 'grad1', 'grad2'):
        _fixture_close(r[k], fx[pre + 'proposed/' + k], 'proposed ' + k)
    q, wm = LC.pseudo_label_reference(list(torch.from_numpy(fx[pre + 'ensemble/passes'])), 2.0)
    _fixture_close(q, fx[pre + 'ensemble/pseudo'], 'ensemble pseudo label')
    _fixture_close(wm, fx[pre + 'ensemble/wmap'], 'ensemble weight map')
    lab, sure = LC.label_reference(z1)
    assert torch.equal(lab[sure], torch.from_numpy(fx[pre + 'labels'])[sure]) and sure.float().mean() > 0.999


# ------------------------------------------------------------------------------- the reference against itself and the oracle
@pytest.mark.parametrize('case', [c for c in LC.CASES if c.h * c.w <= 4100], ids=lambda c: LC.case_id(c))
def test_shared_statistics_equal_one_autograd_pass(case):
    """reference() differentiates the statistics once per case and applies the chain rule per form; one plain autograd pass
    over the whole expression gives the same value and gradient to float64 rounding"""
    for form in LC.FORMS:
        (v, g), (dv, dg) = LC.reference(case, form), LC.direct(form, LC.operands(case))
        assert (v - dv).abs().max().item() <= 1e-12 * max(1.0, dv.abs().max().item()), form
        assert (g - dg).abs().max().item() <= 1e-12 * max(1e-30, dg.abs().max().item()) + 1e-18, form


@pytest.mark.parametrize('case', LC.CASES, ids=IDS)
def test_fp32_oracle_within_half_the_bound(case):
    """plain fp32 (aten on the CPU) needs at most half of the GPU bound on these inputs"""
    o = LC.operands(case)
    worst = (0.0, '')
    for form in LC.FORMS:
        z = o.z.clone().requires_grad_(True)
        v, _ = LC.run_form(oracle, form, o._replace(z=z))
        LC.backward_of(v)
        rv, rg = LC.reference(case, form)
        worst = max(worst, (LC.rel_err(v, rv), form), (LC.rel_err(z.grad, rg), form + ' grad'))
    for form in LC.PROB_FORMS:
        x, t = LC.prob_input(case)
        x = x.clone().requires_grad_(True)
        v = oracle.DiceLoss(**LC.PROB_FORMS[form])(x, t)
        LC.backward_of(v)
        rv, rg = LC.prob_reference(case, form)
        worst = max(worst, (LC.rel_err(v, rv), form), (LC.rel_err(x.grad, rg), form + ' grad'))
    st = LC.base(case)[0]
    worst = max(worst, (LC.rel_err(torch.as_tensor(oracle.Dice_fn(o.z, o.t)), torch.tensor(LC.hard_dice_sum(st))), 'Dice_fn'))
    for k, temp in ((1, 1.0), (4, 0.5), (8, 2.0)):
        passes = LC.ensemble_passes(case)[:k]
        (q, wm), (rq, rwm) = steps.pseudo_labels(list(passes), temp), LC.pseudo_label_reference(passes, temp)
        worst = max(worst, (LC.rel_err(q, rq), 'pseudo label'), (LC.rel_err(wm, rwm), 'weight map'))
    print('%-16s worst fp32 error %.3f of the GPU bound (%s)' % (LC.case_id(case), worst[0], worst[1]))
    assert worst[0] <= HALF, worst


@pytest.mark.parametrize('case', LC.SATURATION_CASES, ids=lambda c: LC.case_id(c))
def test_fp32_oracle_on_saturated_logits(case):
    """logit differences of +-80 leave plain fp32 within half the bound too"""
    o = LC.operands(case)._replace(z=LC.saturated(case))
    for form in LC.SATURATION_FORMS:
        z = o.z.clone().requires_grad_(True)
        v, _ = LC.run_form(oracle, form, o._replace(z=z))
        LC.backward_of(v)
        rv, rg = LC.direct(form, o)
        assert bool(torch.isfinite(rv).all()) and bool(torch.isfinite(rg).all()), form
        assert LC.rel_err(v, rv) <= HALF and LC.rel_err(z.grad, rg) <= HALF, form


def _gaps(per):
    s = torch.sort(per).values
    return float('inf') if s.numel() < 2 else (s[1:] - s[:-1]).min().item()


@pytest.mark.parametrize('case', LC.CASES, ids=IDS)
def test_inputs_allow_exact_comparisons(case):
    o = LC.operands(case)
    st1, stw, _ = LC.base(case)
    hw = case.h * case.w
    if (case.n, case.h, case.w) != LC.BATCH_GEOMETRY:
        # the per-image vectors whose argsort the GPU test compares: CE + Dice, CE alone, Dice alone
        for what, per in (('cemdice', LC.per_image_loss(stw, hw, *LC.CEDICE)), ('ce', LC.per_image_loss(stw, hw, 1.0, 0.0)),
                          ('dice', LC.per_image_loss(st1, hw, 0.0, 1.0))):
            assert _gaps(per) > LC.MIN_GAP, (what, per.tolist())
    p = torch.softmax(o.z.double(), 1)
    assert ((p[:, 1] - 0.5).abs() >= LC.P1_MARGIN).all()
    _, sure = LC.label_reference(o.z)
    assert 1.0 - sure.double().mean().item() <= LC.TOP2_CAP


@pytest.mark.parametrize('c', LC.COTEACH_CLASSES)
def test_coteach_inputs_allow_exact_argsorts(c):
    for n in sorted(set(n for n, _ in LC.COTEACH_SPLITS)):
        o = LC.coteach_operands(n, c)
        for z in (o.z1, o.z2):
            assert ((torch.softmax(z.double(), 1)[:, 1] - 0.5).abs() >= LC.P1_MARGIN).all()
        assert LC.coteach_min_gap(o) > LC.MIN_GAP, (n, c)
        # the two networks rank the images differently: the cross selection is not the own selection
        r = LC.coteach_reference(o.z1, o.z2, o.t1, o.t2, 1, 1, 1.0, 1.0)
        assert r['argsort1'].tolist() != r['argsort2'].tolist()


def test_coteach_reference_is_the_oracle_selection():
    """the float64 selection against the fp32 restatements of the reference: oracle.Coteachingloss_* and
    oracle.steps.proposed_losses, at the splits the GPU test runs (weightimage where the reference's broadcast is defined)"""
    c = 4
    for n, keep in LC.COTEACH_SPLITS:
        if keep >= n:
            continue                # the oracle's slices give empty drop sets there: NaN means, compared on the GPU side
        o = LC.coteach_operands(n, c)
        fr = 1.0 - (keep + 0.5) / n                                 # int((1 - fr) n) == keep
        assert int((1 - fr) * n) == keep
        for variant, cname in ((1, 'Coteachingloss_dropimage'), (2, 'Coteachingloss_weightimage')):
            a1, a2 = o.z1.clone().requires_grad_(True), o.z2.clone().requires_grad_(True)
            l1, l2 = getattr(oracle, cname)(weight=0.7, reduction='none')(a1, a2, o.t1, fr)
            (l1 + l2).backward()
            r = LC.coteach_reference(o.z1, o.z2, o.t1, o.t1, variant, keep, 0.7, 1.0)
            for got, k in ((l1, 'loss1'), (l2, 'loss2'), (a1.grad, 'grad1'), (a2.grad, 'grad2')):
                assert LC.rel_err(got, r[k]) <= HALF, (n, keep, cname, k)
        w, cw = torch.tensor(LC.CEDICE), torch.tensor(o.class_w)
        for rate in (0.0, 0.3, 1.0):
            a1, a2 = o.z1.clone().requires_grad_(True), o.z2.clone().requires_grad_(True)
            l1, l2, i1, i2, _, _ = steps.proposed_losses(oracle.CEMDiceLossImage(w, cw, cw), oracle.MulticlassMSELoss('none'),
                                                         a1, a2, o.t1, o.t2, o.q1, o.wm1, o.q2, o.wm2, rate,
                                                         segcor_weight=(1.0, 10.0), keep=keep)
            l1.backward()
            l2.backward()
            # net 1 is scored against targets2 / pseudo2 / wmap2 (trainchaos_proposed_30cases1labeled.py:303, :311)
            r = LC.coteach_reference(o.z1, o.z2, o.t2, o.t1, 0, keep, LC.CEDICE[0], LC.CEDICE[1], o.class_w, rate=rate,
                                     w_seg=1.0, w_cor=10.0, q1=o.q2, wm1=o.wm2, q2=o.q1, wm2=o.wm1)
            assert i1.tolist() == r['argsort1'].tolist() and i2.tolist() == r['argsort2'].tolist()
            for got, k in ((l1, 'loss1'), (l2, 'loss2'), (a1.grad, 'grad1'), (a2.grad, 'grad2')):
                assert LC.rel_err(got, r[k]) <= HALF, (n, keep, rate, k)
