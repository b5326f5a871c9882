"""Kernel-level net under the fused loss kernels of csrc/loss.hip (-m gpu): every class count 2 .. 8 on every block split
(1, 2, 3 blocks per image and the 64-block cap), N = 1 and N = 260, against the float64 reference of tests/loss_cases.py (made
binding on the host by tests/test_loss_reference_host.py).

  through the drop-in modules   value and input gradient of every loss form, the eight statistics, the argsort, Dice_fn,
                                inference.label_map and pseudo_label_ensemble
  through the C ABI             every entry point with batch strides larger than dense, every tensor a view into a NaN-patterned
                                guarded buffer, workspaces sized exactly by the library's own queries: bit for bit the dense
                                result, gaps and guards intact, every workspace word written
  co-teaching finalize          keep / drop splits beyond 2 of 4, D = 0, keep > N, keep = 0, a NaN image
  saturation, determinism

Bounds: integers (labels, argsort, the integer statistics) are exact; floating values and gradients
max |got - ref| <= 1e-4 max |ref| + 1e-9, the project's loss bound (`close` of test_gpu_losses.py), of which plain fp32 needs
less than a twentieth on these inputs (test_loss_reference_host.py).  Run with -s for the largest error of each test.

Largest errors measured on an MI355X, in units of that bound: module values, gradients and statistics 0.023 (dice_none grad,
3x1x1-c3); pseudo-label ensemble 0.38 (two-class weight map, K = 1, T = 0.5, 1x362x362: 1 - 4 q0 q1 next to a cancellation), else
0.004; strided C-ABI calls 0.005; co-teaching selection 0.017; saturated logits 0.012.

Mutation check (not part of the suite): with `partials[(n * bpi + b) * NS + k]` of seg_stats_mc_kernel written without `+ b`,
59 of the 111 tests here fail (every C >= 3 case with more than one block per image) and none of test_gpu_losses.py or
test_gpu_multiclass.py does."""
import ctypes

import pytest
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu

IDS = [LC.case_id(c) for c in LC.CASES]


class Worst(object):
    """collects errors in units of the bound, asserts each, prints the largest with -s"""

    def __init__(self, title):
        self.title, self.worst = title, (0.0, '')

    def close(self, got, ref, what):
        e = LC.rel_err(got, ref)
        self.worst = max(self.worst, (e, what))
        assert e <= 1.0, '%s %s: %.3f of the bound' % (self.title, what, e)

    def report(self):
        print('%-28s largest error %.4f of the bound (%s)' % (self.title, self.worst[0], self.worst[1]))


def _on(o, dev, z=None):
    """the operands on the device, the logits a fresh leaf"""
    mv = lambda x: x.to(dev) if isinstance(x, torch.Tensor) else x
    return LC.Operands(*[mv(x) for x in o])._replace(z=(o.z if z is None else z).to(dev).requires_grad_(True))


def _is_batch(case):
    return (case.n, case.h, case.w) == LC.BATCH_GEOMETRY


# ------------------------------------------------------------------------------------------------ the drop-in modules
@pytest.mark.parametrize('case', LC.CASES, ids=IDS)
def test_modules_value_gradient_statistics(dev, case):
    from aide_amd import utils as U
    o, hw = LC.operands(case), case.h * case.w
    w = Worst(LC.case_id(case))
    st1, stw, _ = LC.base(case)
    for form in LC.FORMS:
        d = _on(o, dev)
        v, m = LC.run_form(U, form, d)
        LC.backward_of(v)
        rv, rg = LC.reference(case, form)
        w.close(v, rv, form)
        w.close(d.z.grad, rg, form + ' grad')
        name, kw, kind = LC.FORM_TABLE[form]
        sf = LC.statistics_form(name, kw(o), kind == 'onehot')
        if sf is None:
            continue
        # the fused statistics behind the value: op.last
        cw, w_ce, w_dice, smooth, _ = sf
        st = st1 if cw is None else stw
        got = m.last['stats'].cpu()
        assert got.shape == (case.n, 8)
        for k, sname in enumerate(LC.STAT_NAMES):
            if sname in ('T', 'hP', 'hI') or (sname == 'Wsum' and cw is None):
                assert torch.equal(got[:, k], st[sname]), (form, sname)          # sums of integers: exact
            else:
                w.close(got[:, k], st[sname], '%s stats %s' % (form, sname))
        per_ref = LC.per_image_loss(st, hw, w_ce, w_dice, smooth)
        per = m.last['per_image'].cpu()
        w.close(per, per_ref, form + ' per image')
        order = m.last['argsort'].cpu()
        if _is_batch(case):
            assert sorted(order.tolist()) == list(range(case.n)), form
            assert bool((per[order][1:] >= per[order][:-1]).all()), form          # in the kernel's own values
        elif smooth == 1.0:          # the per-image vectors whose gaps the host test asserts
            assert order.tolist() == LC.stable_argsort(per_ref).tolist(), form
    for form, kw in LC.PROB_FORMS.items():
        x, t = LC.prob_input(case)
        x = x.to(dev).requires_grad_(True)
        v = U.DiceLoss(**kw)(x, t.to(dev))
        LC.backward_of(v)
        rv, rg = LC.prob_reference(case, form)
        w.close(v, rv, form)
        w.close(x.grad, rg, form + ' grad')
    w.report()


@pytest.mark.parametrize('case', LC.CASES, ids=IDS)
def test_dice_fn_label_map_ensemble(dev, case):
    from aide_amd import utils as U
    from aide_amd.inference import label_map
    from aide_amd.utils.coteach_loss import pseudo_label_ensemble
    o = LC.operands(case)
    w = Worst(LC.case_id(case))
    z = o.z.to(dev)
    w.close(U.Dice_fn(z, o.t.to(dev)), torch.tensor(LC.hard_dice_sum(LC.base(case)[0])), 'Dice_fn')
    lab, sure = LC.label_reference(o.z)
    got = label_map(z).cpu()
    assert got.dtype == torch.int64 and torch.equal(got[sure], lab[sure])
    passes = [p.to(dev) for p in LC.ensemble_passes(case)]
    for k in (1, 4, 8):
        for temp in (1.0, 0.5, 2.0):
            q, wm = pseudo_label_ensemble(passes[:k], temperature=temp)
            rq, rwm = LC.pseudo_label_reference(None, temp, mean=LC.ensemble_mean(case, k))
            w.close(q, rq, 'pseudo label K=%d T=%g' % (k, temp))
            w.close(wm, rwm, 'weight map K=%d T=%g' % (k, temp))
    w.report()


# ------------------------------------------------------------------------------------------------ the C ABI
class Slab(object):
    """n rows of `per` elements with `pad` untouched elements behind each row, inside a NaN-patterned guarded buffer: .t is the
    [n, per] view a kernel reads or writes with batch stride .bs"""

    def __init__(self, dev, n, per, pad=0, dtype=torch.float32, src=None):
        words = 2 if dtype in (torch.int64, torch.float64) else 1
        self.per, self.bs = per, per + pad
        self.numel = n * self.bs * words                     # fp32 words
        self.buf, flat = LC.guarded(self.numel, LC.LEAD, dev)
        self.grid = flat.view(dtype).view(n, self.bs)
        self.t = self.grid[:, :per]
        if src is not None:
            self.t.copy_(src.reshape(n, per).to(dev))

    def intact(self):
        """guard words on both sides and the gaps between the rows still hold the pattern"""
        return LC.guards_intact(self.buf, LC.LEAD, self.numel) and LC.all_pattern(self.grid[:, self.per:])

    def fully_written(self):
        return not bool((self.t.contiguous().view(torch.int32) == LC.NAN_BITS).any())


def _abi_run(case, dev, g_stride, pads):
    """every entry point of loss.hip once, on Slabs with the given pads (all zero: the dense call) -> (dict of results,
    list of (name, Slab) to inspect, the two workspaces)"""
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    from aide_amd.utils import _seg
    o = LC.operands(case)
    n, c, hw = case.n, case.c, case.h * case.w
    cw = _seg.class_w_array(o.class_w, c)
    red = 2 if g_stride else 0
    ng = n if g_stride else 1
    f64, i64 = torch.float64, torch.int64
    S, slabs = {}, []

    def slab(name, rows, per, pad=0, dtype=torch.float32, src=None):
        S[name] = Slab(dev, rows, per, pad, dtype, src)
        slabs.append((name, S[name]))
        return S[name]

    z = slab('z', n, c * hw, pads['l'], src=o.z)
    t = slab('t', n, hw, pads['t'], i64, o.t)
    q = slab('q', n, c * hw, pads['p'], src=o.pseudo)
    wm = slab('wm', n, hw, pads['w'], src=o.wmap)
    oh = slab('onehot', n, c * hw, pads['t'] + 8, src=LC.onehot(o.t, c))
    gramp = lambda k: torch.linspace(0.5, 1.5, k)
    sp = stream_ptr()

    # statistics -> finalize -> backward
    ws = slab('partials', 1, lib.aide_seg_loss_ws_bytes(n, hw) // 8, 0, f64)
    check(lib.aide_seg_stats(ptr(z.t), z.bs, ptr(t.t), t.bs, cw, c, LC.IGNORE, ptr(q.t), q.bs, ptr(wm.t), wm.bs, n, hw,
                             ptr(ws.t), sp), 'seg_stats')
    stats, out = slab('stats', 1, n * 8, 0, f64), slab('out', 1, ng)
    per, idx, coef, hard = slab('per_image', 1, n), slab('idx', 1, n, 0, i64), slab('coef', 1, 3 * n), slab('hard', 1, 1)
    check(lib.aide_seg_loss_finalize(ptr(ws.t), n, hw, red, LC.CEDICE[0], LC.CEDICE[1], 1.0, ptr(stats.t), ptr(out.t),
                                     ptr(per.t), ptr(idx.t), ptr(coef.t), ptr(hard.t), sp), 'seg_loss_finalize')
    coef_out = coef.t.clone()
    coef.t[0, 2 * n:] = 0.25                 # a consistency coefficient, as coteach_finalize writes: the backward reads q and wm
    g = slab('gout', 1, ng, src=gramp(ng))
    dl = slab('dlogits', n, c * hw, pads['d'])
    check(lib.aide_seg_loss_bwd(ptr(z.t), z.bs, ptr(t.t), t.bs, cw, c, LC.IGNORE, ptr(q.t), q.bs, ptr(wm.t), wm.bs, n, hw,
                                ptr(stats.t), ptr(coef.t), 1.0, ptr(g.t), g_stride, ptr(dl.t), dl.bs, sp), 'seg_loss_bwd')
    # cross-entropy map and consistency map, forward and backward
    ce = slab('ce_map', n, hw)
    check(lib.aide_ce_map(ptr(z.t), z.bs, ptr(t.t), t.bs, cw, c, LC.IGNORE, n, hw, ptr(ce.t), None, None, 0, sp), 'ce_map')
    gmap = slab('g_ce', n, hw, src=gramp(n * hw))
    dce = slab('d_ce', n, c * hw, pads['d'] + 4)
    check(lib.aide_ce_map(ptr(z.t), z.bs, ptr(t.t), t.bs, cw, c, LC.IGNORE, n, hw, None, ptr(gmap.t), ptr(dce.t), dce.bs, sp),
          'ce_map bwd')
    mse = slab('mse_map', n, c * hw)
    check(lib.aide_mse_map(ptr(z.t), z.bs, ptr(q.t), q.bs, c, n, hw, ptr(mse.t), None, None, 0, sp), 'mse_map')
    gmse = slab('g_mse', n, c * hw, src=gramp(n * c * hw))
    dmse = slab('d_mse', n, c * hw, pads['d'] + 12)
    check(lib.aide_mse_map(ptr(z.t), z.bs, ptr(q.t), q.bs, c, n, hw, None, ptr(gmse.t), ptr(dmse.t), dmse.bs, sp), 'mse_map bwd')
    # label map, pseudo-label ensemble
    lab = slab('labels', n, hw, 0, i64)
    check(lib.aide_label_map(ptr(z.t), z.bs, c, n, hw, ptr(lab.t), sp), 'label_map')
    passes = [slab('pass%d' % k, n, c * hw, pads['l'], src=p) for k, p in enumerate(LC.ensemble_passes(case)[:3])]
    arr = (ctypes.c_void_p * 3)(*[p.t.data_ptr() for p in passes])
    pl, pwm = slab('pl', n, c * hw), slab('pl_wm', n, hw)
    check(lib.aide_pseudo_label(arr, 3, c, passes[0].bs, n, hw, 0.5, ptr(pl.t), ptr(pwm.t), sp), 'pseudo_label')
    # one Dice term per class on one-hot targets, and the probability-input form (C = 1)
    dws = slab('dice_ws', 1, lib.aide_dice_terms_ws_bytes(n, hw, c) // 8, 0, f64)
    dper, dout = slab('dice_per', 1, n), slab('dice_out', 1, ng)
    check(lib.aide_dice_terms_fwd(ptr(z.t), z.bs, ptr(oh.t), oh.bs, n, hw, c, cw, 0.5, red, ptr(dws.t), ptr(dper.t),
                                  ptr(dout.t), sp), 'dice_terms_fwd')
    ddx = slab('dice_dx', n, c * hw, pads['d'] + 20)
    check(lib.aide_dice_terms_bwd(ptr(z.t), z.bs, ptr(oh.t), oh.bs, n, hw, c, cw, 0.5, red, ptr(dws.t), ptr(g.t), ptr(ddx.t),
                                  ddx.bs, sp), 'dice_terms_bwd')
    x1, t1 = LC.prob_input(case)
    px, pt = slab('prob', n, hw, pads['l'] + 4, src=x1), slab('prob_t', n, hw, pads['t'] + 4, src=t1)
    pws = slab('prob_ws', 1, lib.aide_dice_terms_ws_bytes(n, hw, 1) // 8, 0, f64)
    pper, pout = slab('prob_per', 1, n), slab('prob_out', 1, ng)
    check(lib.aide_dice_terms_fwd(ptr(px.t), px.bs, ptr(pt.t), pt.bs, n, hw, 1, None, 1.0, red, ptr(pws.t), ptr(pper.t),
                                  ptr(pout.t), sp), 'dice_terms_fwd prob')
    pdx = slab('prob_dx', n, hw, pads['d'] + 28)
    check(lib.aide_dice_terms_bwd(ptr(px.t), px.bs, ptr(pt.t), pt.bs, n, hw, 1, None, 1.0, red, ptr(pws.t), ptr(g.t),
                                  ptr(pdx.t), pdx.bs, sp), 'dice_terms_bwd prob')
    am = slab('argmax', n, hw, 0, i64)
    check(lib.aide_onehot_argmax(ptr(oh.t), oh.bs, n, c, hw, ptr(am.t), sp), 'onehot_argmax')
    torch.cuda.synchronize()
    outputs = ('partials', 'stats', 'out', 'per_image', 'idx', 'hard', 'dlogits', 'ce_map', 'd_ce', 'mse_map', 'd_mse',
               'labels', 'pl', 'pl_wm', 'dice_ws', 'dice_per', 'dice_out', 'dice_dx', 'prob_ws', 'prob_per', 'prob_out',
               'prob_dx', 'argmax')
    res = dict((k, S[k].t.contiguous().clone()) for k in outputs)
    res['coef'] = coef_out
    return res, slabs, (ws, dws, pws)


_DENSE = {}


def _abi_dense(case, dev, g_stride):
    """the dense call's results, computed once per (case, g_stride) and left unchanged"""
    if (case, g_stride) not in _DENSE:
        res, slabs, _ = _abi_run(case, dev, g_stride, dict(l=0, t=0, p=0, w=0, d=0))
        assert all(s.intact() for _, s in slabs)
        _DENSE[(case, g_stride)] = res
    return _DENSE[(case, g_stride)]


@pytest.mark.parametrize('g_stride', [0, 1])
@pytest.mark.parametrize('case', LC.ABI_CASES, ids=lambda c: LC.case_id(c))
def test_abi_strided_calls_in_guarded_buffers(dev, case, g_stride):
    """batch strides larger than dense, a different pad per tensor; g_stride 0 (one upstream scalar, reduction mean) and 1 (one
    per image, the per-image reduction)"""
    dense = _abi_dense(case, dev, g_stride)
    res, slabs, workspaces = _abi_run(case, dev, g_stride, dict(l=24, t=40, p=56, w=8, d=72))
    for name, s in slabs:
        assert s.intact(), name                      # nothing written outside a view: not into a gap, not past either end
    for ws in workspaces:
        assert ws.fully_written()                    # sized exactly by the library's own query, and all of it used
    for k, v in res.items():
        assert torch.equal(v.view(torch.int32), dense[k].view(torch.int32)), k         # bit for bit
    # and the dense call is the operator: the fused value and the maps against the float64 reference
    w = Worst(LC.case_id(case))
    o = LC.operands(case)
    rv, _ = LC.reference(case, 'cemdice_image' if g_stride else 'cemdice_mean')
    w.close(dense['out'].view(-1), rv.view(-1), 'seg loss')
    st = LC.statistics(o.z.double(), o.t, o.class_w, o.pseudo, o.wmap)      # with the consistency sum M this time
    got = dense['stats'].view(case.n, 8).cpu()
    for k, sname in enumerate(LC.STAT_NAMES):
        if sname in ('T', 'hP', 'hI'):
            assert torch.equal(got[:, k], st[sname]), sname
        else:
            w.close(got[:, k], st[sname], 'stats ' + sname)
    w.close(dense['ce_map'].view(o.t.shape), LC.reference(case, 'ce_none')[0], 'ce map')
    w.close(dense['mse_map'].view(o.z.shape), (torch.softmax(o.z.double(), 1) - o.pseudo.double()) ** 2, 'mse map')
    lab, sure = LC.label_reference(o.z)
    assert torch.equal(dense['labels'].view(o.t.shape).cpu()[sure], lab[sure])
    assert torch.equal(dense['argmax'].view(o.t.shape).cpu(), LC.index_targets(o.t))
    w.report()


# ------------------------------------------------------------------------------------------------ co-teaching finalize
def _coteach(dev, o, variant, keep, w_ce, w_dice, class_w=None, rate=0.0, w_seg=1.0, w_cor=0.0, pseudo=False, z1=None):
    """_seg.coteach_loss on the device -> dict shaped as LC.coteach_reference returns it"""
    from aide_amd.utils import _seg
    a1 = (o.z1 if z1 is None else z1).to(dev).requires_grad_(True)
    a2 = o.z2.to(dev).requires_grad_(True)
    ps = [x.to(dev) for x in (o.q1, o.wm1, o.q2, o.wm2)] if pseudo else [None] * 4
    l1, l2, last = _seg.coteach_loss(a1, a2, o.t1.to(dev), o.t2.to(dev), variant, keep, w_ce, w_dice, 1.0, rate, w_seg, w_cor,
                                     ps[0], ps[1], ps[2], ps[3], class_w)
    l1.backward()
    assert a2.grad is None                   # loss 1 only reaches net 1's logits
    l2.backward()
    return dict(loss1=l1.detach(), loss2=l2.detach(), grad1=a1.grad, grad2=a2.grad, per_image1=last['per_image1'],
                per_image2=last['per_image2'], argsort1=last['argsort1'], argsort2=last['argsort2'])


def _coteach_compare(w, got, ref, what):
    for k in ('argsort1', 'argsort2'):
        assert got[k].cpu().tolist() == ref[k].tolist(), (what, k)
    for k in ('loss1', 'loss2', 'per_image1', 'per_image2', 'grad1', 'grad2'):
        w.close(got[k], ref[k], '%s %s' % (what, k))


@pytest.mark.parametrize('c', LC.COTEACH_CLASSES)
@pytest.mark.parametrize('n,keep', LC.COTEACH_SPLITS)
def test_coteach_finalize_splits(dev, n, keep, c):
    """the three variants of coteach_finalize_kernel against the float64 selection: both losses, both argsorts (exact), both
    per-image vectors and both logit gradients.  An empty drop set makes the proposed step's loss NaN (the reference's mean of
    an empty set); its gradient stays finite and is compared."""
    o = LC.coteach_operands(n, c)
    w = Worst('coteach N=%d keep=%d C=%d' % (n, keep, c))
    for variant in (1, 2):          # Coteachingloss_dropimage / _weightimage: weight 0.7 on the cross-entropy, unit class weights
        got = _coteach(dev, o, variant, keep, 0.7, 1.0)
        ref = LC.coteach_reference(o.z1, o.z2, o.t1, o.t2, variant, keep, 0.7, 1.0)
        _coteach_compare(w, got, ref, 'variant %d' % variant)
    for rate in (0.0, 0.3, 1.0):    # the proposed inline step, pseudo label and weight map present
        got = _coteach(dev, o, 0, keep, LC.CEDICE[0], LC.CEDICE[1], o.class_w, rate, 1.0, 10.0, pseudo=True)
        ref = LC.coteach_reference(o.z1, o.z2, o.t1, o.t2, 0, keep, LC.CEDICE[0], LC.CEDICE[1], o.class_w, 1.0, rate, 1.0,
                                   10.0, o.q1, o.wm1, o.q2, o.wm2)
        assert bool(torch.isnan(ref['loss1'])) == (keep >= n)
        _coteach_compare(w, got, ref, 'proposed rate %g' % rate)
    w.report()


@pytest.mark.parametrize('c', LC.COTEACH_CLASSES)
def test_coteach_modules_and_edges(dev, c):
    from aide_amd import utils as U
    from aide_amd.utils.coteach_loss import CoTeachingProposedLoss
    n = 5
    o = LC.coteach_operands(n, c)
    w = Worst('coteach modules C=%d' % c)
    d = dict((k, getattr(o, k).to(dev)) for k in ('t1', 't2', 'q1', 'wm1', 'q2', 'wm2'))
    # the modules above _seg.coteach_loss: int((1 - 0.3) 5) = 3 kept, 2 dropped (weightimage: 4 kept, 1 dropped)
    for variant, cname, fr, keep in ((1, 'Coteachingloss_dropimage', 0.3, 3), (2, 'Coteachingloss_weightimage', 0.1, 4)):
        a1, a2 = o.z1.to(dev).requires_grad_(True), o.z2.to(dev).requires_grad_(True)
        op = getattr(U, cname)(weight=0.7, reduction='none')
        l1, l2 = op(a1, a2, d['t1'], fr)
        (l1 + l2).backward()
        ref = LC.coteach_reference(o.z1, o.z2, o.t1, o.t1, variant, keep, 0.7, 1.0)
        got = dict(loss1=l1, loss2=l2, grad1=a1.grad, grad2=a2.grad, **op.last)
        _coteach_compare(w, got, ref, cname)
    # the proposed loss scores net 1 against targets 2 / pseudo 2 / weight map 2
    a1, a2 = o.z1.to(dev).requires_grad_(True), o.z2.to(dev).requires_grad_(True)
    op = CoTeachingProposedLoss(cediceweight=LC.CEDICE, ceclassweight=o.class_w, segcor_weight=(1.0, 10.0), keep=3)
    l1, l2, i1, i2 = op(a1, a2, d['t1'], d['t2'], d['q1'], d['wm1'], d['q2'], d['wm2'], 0.3)
    (l1 + l2).backward()
    ref = LC.coteach_reference(o.z1, o.z2, o.t2, o.t1, 0, 3, LC.CEDICE[0], LC.CEDICE[1], o.class_w, 1.0, 0.3, 1.0, 10.0,
                               o.q2, o.wm2, o.q1, o.wm1)
    got = dict(loss1=l1, loss2=l2, grad1=a1.grad, grad2=a2.grad, **op.last)
    assert torch.equal(i1, op.last['argsort1']) and torch.equal(i2, op.last['argsort2'])
    _coteach_compare(w, got, ref, 'CoTeachingProposedLoss')
    # keep = 0: the mean of an empty keep set is NaN, as in the reference; the argsorts are still the reference's
    for variant in (0, 1, 2):
        got = _coteach(dev, o, variant, 0, 0.7, 1.0, pseudo=variant == 0, rate=0.3, w_cor=10.0)
        assert bool(torch.isnan(got['loss1'])) and bool(torch.isnan(got['loss2'])), variant
        ref = LC.coteach_reference(o.z1, o.z2, o.t1, o.t2, 1, 0, 0.7, 1.0)
        assert got['argsort1'].cpu().tolist() == ref['argsort1'].tolist()
        assert got['argsort2'].cpu().tolist() == ref['argsort2'].tolist()
    # one image with a NaN logit: its loss is NaN, it sorts last, and every idx slot is still a valid index
    z1 = o.z1.clone()
    z1[1, 0, 3, 3] = float('nan')
    got = _coteach(dev, o, 1, 2, 0.7, 1.0, z1=z1)
    ref = LC.coteach_reference(z1, o.z2, o.t1, o.t2, 1, 2, 0.7, 1.0)
    order = got['argsort1'].cpu().tolist()
    assert order[-1] == 1 and sorted(order) == list(range(n)) and order == ref['argsort1'].tolist()
    assert got['argsort2'].cpu().tolist() == ref['argsort2'].tolist()
    assert bool(torch.isnan(got['per_image1'][1]))
    w.close(got['per_image1'], ref['per_image1'], 'NaN image: per image')
    w.close(got['loss2'], ref['loss2'], 'NaN image: loss 2')       # net 2 is trained on net 1's two smallest: finite
    w.report()


# ------------------------------------------------------------------------------------------------ saturation, determinism
@pytest.mark.parametrize('case', LC.SATURATION_CASES, ids=lambda c: LC.case_id(c))
def test_saturated_logits(dev, case):
    """logit differences of +-80: soft-max terms under- and overflow towards 0 and 1; values and gradients stay finite and
    within the bound on the statistics / finalize / backward path, the two maps and the per-class Dice terms"""
    from aide_amd import utils as U
    o = LC.operands(case)._replace(z=LC.saturated(case))
    w = Worst('saturated ' + LC.case_id(case))
    for form in LC.SATURATION_FORMS:
        d = _on(o, dev)
        v, _ = LC.run_form(U, form, d)
        LC.backward_of(v)
        assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(d.z.grad).all()), form
        rv, rg = LC.direct(form, o)
        w.close(v, rv, form)
        w.close(d.z.grad, rg, form + ' grad')
    ignored = torch.full_like(o.t, LC.IGNORE).to(dev)
    assert bool(torch.isnan(U.CrossEntropyLoss2d(reduction='mean')(o.z.to(dev), ignored)))      # 0 / 0, as torch
    w.report()


def test_determinism_and_batch_permutation(dev):
    """C = 5 on two blocks per image: two runs are bit-identical (fixed-order reductions, no atomics) and permuting the batch
    permutes the per-image losses bit-exactly (test_full_size_properties holds the same for two classes)"""
    from aide_amd import utils as U
    case = LC.Case(3, 46, 50, 5)
    assert case in LC.CASES
    o = LC.operands(case)

    def run(z, t):
        z = z.to(dev).requires_grad_(True)
        m = U.CEMDiceLossImage(torch.tensor(LC.CEDICE), torch.tensor(o.class_w), torch.tensor(o.class_w))
        v = m(z, t.to(dev))
        LC.backward_of(v)
        return v.detach(), z.grad, m.last['stats'].clone()
    a, b = run(o.z, o.t), run(o.z, o.t)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    perm = torch.tensor([2, 0, 1])
    p = run(o.z[perm].contiguous(), o.t[perm].contiguous())
    assert torch.equal(p[0], a[0][perm.to(dev)]) and torch.equal(p[2], a[2][perm.to(dev)])
