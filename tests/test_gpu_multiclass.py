"""-m gpu: num_classes = 3 .. 8 through the drop-in modules (the soft-max templates of csrc/loss.hip and
csrc/coteach_ext.hip, the head kernels for K <= 8), against the values and gradients of the real reference (tests/golden/g17_multiclass.npz, oracle/gen_golden.py::g17_multiclass).
fp32 tolerance 1e-4 relative (north star: 1e-3); labels and selection indices exact."""
import os

import numpy as np
import pytest
import torch

from multiclass_cases import loss_cases, targets_of, upstream

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def close(a, b, rtol=1e-4, what=''):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)).double()
    b = torch.as_tensor(np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b)).double()
    err = (a - b).abs().max().item()
    assert err <= rtol * (b.abs().max().item() + 1e-12) + 1e-9, '%s: err %.3e (scale %.3e)' % (what, err, b.abs().max().item())


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLD, 'g17_multiclass.npz'))


@pytest.mark.parametrize('C', [3, 5, 8])
def test_golden_multiclass_losses(dev, fx, C):
    from aide_amd import utils as U
    pre = 'c%d/' % C
    z1 = torch.from_numpy(fx[pre + 'z1']).to(dev)
    for key, lname, kw, kind in loss_cases(fx, pre):
        zz = z1.clone().requires_grad_(True)
        v = getattr(U, lname)(**kw)(zz, targets_of(fx, pre, kind, C).to(dev))
        ((v * upstream(v)).sum() if v.dim() else v).backward()
        close(v, fx[pre + key], what='%d %s' % (C, key))
        close(zz.grad, fx[pre + key + '/grad'], what='%d %s grad' % (C, key))
    t = torch.from_numpy(fx[pre + 'targets']).to(dev)
    close(U.Dice_fn(z1, t), fx[pre + 'Dice_fn'], what='Dice_fn')
    # the consistency term with the caller-side mean (trainchaos_proposed_30cases1labeled.py:311-313)
    zz = z1.clone().requires_grad_(True)
    pseudo, wmap = torch.from_numpy(fx[pre + 'pseudo']).to(dev), torch.from_numpy(fx[pre + 'wmap']).to(dev)
    v = (wmap * U.MulticlassMSELoss(reduction='none')(zz, pseudo)).mean()
    v.backward()
    close(v, fx[pre + 'mse_wm_mean'], what='mse')
    close(zz.grad, fx[pre + 'mse_wm_mean/grad'], what='mse grad')


@pytest.mark.parametrize('C', [3, 5, 8])
@pytest.mark.parametrize('cname', ['Coteachingloss_dropimage', 'Coteachingloss_weightimage'])
@pytest.mark.parametrize('fr', [0.25, 0.5])
def test_golden_multiclass_coteaching(dev, fx, C, cname, fr):
    from aide_amd import utils as U
    pre = 'c%d/' % C
    a1 = torch.from_numpy(fx[pre + 'z1']).to(dev).requires_grad_(True)
    a2 = torch.from_numpy(fx[pre + 'z2']).to(dev).requires_grad_(True)
    t = torch.from_numpy(fx[pre + 'targets']).to(dev)
    l1, l2 = getattr(U, cname)(weight=1.0, reduction='none')(a1, a2, t, fr)
    (l1 + l2).backward()
    key = '%s%s/fr%g' % (pre, cname, fr)
    close(l1, fx[key + '/loss1'], what=key + ' loss1')
    close(l2, fx[key + '/loss2'], what=key + ' loss2')
    close(a1.grad, fx[key + '/grad1'], what=key + ' grad1')
    close(a2.grad, fx[key + '/grad2'], what=key + ' grad2')


@pytest.mark.parametrize('C', [3, 5, 8])
def test_golden_multiclass_proposed_loss_and_ensemble(dev, fx, C):
    """The composite loss of the proposed loop (cross-scored selection, keep 2 of 4, consistency term on the dropped
    images: trainchaos_proposed_30cases1labeled.py:303-321) and the pseudo-label ensemble (:274-288) on C classes."""
    from aide_amd.utils.coteach_loss import CoTeachingProposedLoss, pseudo_label_ensemble
    pre = 'c%d/' % C
    a1 = torch.from_numpy(fx[pre + 'z1']).to(dev).requires_grad_(True)
    a2 = torch.from_numpy(fx[pre + 'z2']).to(dev).requires_grad_(True)
    t = torch.from_numpy(fx[pre + 'targets']).to(dev)
    pseudo, wmap = torch.from_numpy(fx[pre + 'pseudo']).to(dev), torch.from_numpy(fx[pre + 'wmap']).to(dev)
    op = CoTeachingProposedLoss(cediceweight=fx[pre + 'cedice_w'].tolist(), ceclassweight=fx[pre + 'class_w'].tolist(),
                                segcor_weight=(1.0, 10.0), keep=2)
    l1, l2, i1, i2 = op(a1, a2, t, t, pseudo, wmap, pseudo, wmap, 0.3)
    (l1 + l2).backward()
    assert float(fx[pre + 'proposed/min_gap']) > 1e-3
    assert i1.cpu().tolist() == fx[pre + 'proposed/indx1'].tolist()
    assert i2.cpu().tolist() == fx[pre + 'proposed/indx2'].tolist()
    close(l1, fx[pre + 'proposed/loss1'], what='proposed loss1')
    close(l2, fx[pre + 'proposed/loss2'], what='proposed loss2')
    close(a1.grad, fx[pre + 'proposed/grad1'], what='proposed grad1')
    close(a2.grad, fx[pre + 'proposed/grad2'], what='proposed grad2')
    passes = [p.contiguous() for p in torch.from_numpy(fx[pre + 'ensemble/passes']).to(dev)]
    pl, wm = pseudo_label_ensemble(passes, temperature=2.0)
    close(pl, fx[pre + 'ensemble/pseudo'], what='ensemble pseudo label')
    close(wm, fx[pre + 'ensemble/wmap'], rtol=2e-4, what='ensemble weight map')


@pytest.mark.parametrize('C', [3, 5, 8])
def test_multiclass_label_map(dev, fx, C):
    from aide_amd.inference import label_map
    pre = 'c%d/' % C
    z1 = torch.from_numpy(fx[pre + 'z1'])
    lab = label_map(z1.to(dev)).cpu()
    ref = torch.from_numpy(fx[pre + 'labels'])
    # labels agree wherever the two largest probabilities are further apart than the softmax rounding
    p = torch.softmax(z1, dim=1).topk(2, dim=1).values
    sure = (p[:, 0] - p[:, 1]) > 1e-6
    assert torch.equal(lab[sure], ref[sure]) and sure.float().mean() > 0.999
    # exact ties resolve to the first class, as torch.argmax
    z = torch.zeros(1, C, 4, 4)
    z[0, C - 1, 0, 0] = 1.0
    lab = label_map(z.to(dev)).cpu()
    assert lab[0, 0, 0] == C - 1 and lab.sum() == C - 1


@pytest.mark.parametrize('name,C,nin', [('fuseunet3', 3, 2), ('unet4', 4, 1)])
def test_golden_multiclass_models(dev, fx, name, C, nin):
    """fuseunet(num_classes=3) / UNet(num_classes=4): logits, loss, per-image loss, every gradient norm, the head
    gradients element-wise, eval-mode logits and the label map against the real reference."""
    from aide_amd.models_twomodalinputs import fuseunet
    from aide_amd.models_singlemodalinput import UNet
    from aide_amd import utils as U
    from aide_amd.inference import label_map
    torch.manual_seed(2)
    net = (fuseunet if nin == 2 else UNet)(C).to(dev)
    xs = [torch.from_numpy(fx['%s/x%d' % (name, i)]).to(dev) for i in range(nin)]
    t = torch.from_numpy(fx[name + '/targets']).to(dev)
    cw, cdw = torch.from_numpy(fx[name + '/class_w']), torch.from_numpy(fx[name + '/cedice_w'])
    net.train()
    out = net(*xs)
    assert out.shape[1] == C
    loss = U.CEMDiceLoss(cediceweight=cdw, ceclassweight=cw, diceclassweight=cw)(out, t)
    per = U.CEMDiceLossImage(cediceweight=cdw, ceclassweight=cw, diceclassweight=cw)(out.detach(), t)
    loss.backward()
    close(out, fx[name + '/logits'], rtol=1e-3, what='logits')
    close(loss, fx[name + '/loss'], rtol=1e-4, what='loss')
    close(per, fx[name + '/per_image_loss'], rtol=1e-4, what='per-image loss')
    grads = dict((k, p.grad) for k, p in net.named_parameters())
    names = [str(k) for k in fx[name + '/param_names']]
    norms = np.array([grads[k].double().norm().item() for k in names])
    ref = fx[name + '/grad_norms']
    live = ref > 1e-6 * ref.max()              # conv biases in front of a BatchNorm have a zero gradient
    # The only class-count dependent part of the network is the head: its gradients are pinned element-wise.  Below it
    # a 2-image 32x32 batch has BatchNorm populations of 8 values at the bottleneck, where an fp32-noise ReLU mask flip
    # moves a gradient by ~1 % (tests/test_gpu_models.py pins the body element-wise with the masks forced equal; that
    # code path does not depend on the class count), hence the looser bound on the per-parameter norms here.
    assert np.all(np.abs(norms[live] - ref[live]) <= 2e-2 * ref[live]), np.abs(norms[live] / ref[live] - 1).max()
    for k in ('last_conv1.weight', 'last_conv1.bias'):
        close(grads[k], fx['%s/grad/%s' % (name, k)], rtol=1e-3, what=k)
    close(grads[names[0]], fx['%s/grad/%s' % (name, names[0])], rtol=2e-2, what=names[0])
    net.eval()
    with torch.no_grad():
        ev = net(*xs)
    close(ev, fx[name + '/eval_logits'], rtol=1e-3, what='eval logits')
    evr = torch.from_numpy(fx[name + '/eval_logits'])
    top = evr.topk(2, dim=1).values
    sure = (top[:, 0] - top[:, 1]) > 2e-3 * evr.abs().max()
    assert torch.equal(label_map(ev).cpu()[sure], torch.from_numpy(fx[name + '/labels'])[sure])


@pytest.mark.parametrize('C', [3, 5])
def test_golden_multiclass_rank4_operators(dev, fx, C):
    """KLbidirection (utils/coteach_loss.py:85-92), Coteachingloss_dropregionce (:163-196) and _dropimagedroppixel (:198-254)
    on C classes vs the real reference: the KL map and both its gradients; both losses of the two operators and, back-
    propagated separately, their gradients w.r.t. BOTH logit tensors, forget rates 0.25 / 0.5."""
    from aide_amd import utils as U
    pre = 'c%d/' % C
    z1, z2, t = (torch.from_numpy(fx[pre + k]).to(dev) for k in ('z1', 'z2', 'targets'))
    a1, a2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    v = U.KLbidirection(a1, a2)
    close(v, fx[pre + 'KL/map'], rtol=2e-5, what='KL map')
    (v * torch.linspace(0.5, 1.5, v.numel()).view_as(v).to(dev)).sum().backward()
    close(a1.grad, fx[pre + 'KL/grad1'], rtol=2e-5, what='KL grad1')
    close(a2.grad, fx[pre + 'KL/grad2'], rtol=2e-5, what='KL grad2')
    for cname, kw in (('Coteachingloss_dropregionce', dict(scale=0.5, reduction='none')),
                      ('Coteachingloss_dropimagedroppixel', dict(weight=1.0, reduction='none'))):
        for fr in (0.25, 0.5):
            key = '%s%s/fr%g' % (pre, cname, fr)
            for which in (0, 1):
                a1, a2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
                ls = getattr(U, cname)(**kw)(a1, a2, t, fr)
                ref = float(fx[key + '/loss%d' % (which + 1)])
                assert abs(ls[which].item() - ref) < 1e-5 * abs(ref), (key, which, ls[which].item(), ref)
                ls[which].backward()
                for g, gk in ((a1.grad, '/l%d_grad1' % (which + 1)), (a2.grad, '/l%d_grad2' % (which + 1))):
                    gr = fx[key + gk]
                    got = np.zeros_like(gr) if g is None else g.cpu().numpy()
                    # selections may differ from the reference only between values closer than fp32 noise
                    bad = np.abs(got - gr) > 1e-4 * np.abs(gr).max() + 1e-12
                    assert bad.mean() < 2e-4, (key, gk, bad.sum(), np.abs(got - gr).max(), np.abs(gr).max())


def test_class_count_limits(dev):
    from aide_amd import utils as U
    z = torch.randn(2, 9, 8, 8, device=dev)
    t = torch.zeros(2, 8, 8, dtype=torch.long, device=dev)
    with pytest.raises(NotImplementedError):
        U.CrossEntropyLoss2d()(z, t)
    with pytest.raises(RuntimeError):            # nn.CrossEntropyLoss refuses a weight vector of the wrong length too
        U.CrossEntropyLoss2d(weight=torch.tensor([1.0, 2.0, 3.0]))(z[:, :4].contiguous(), t)
    with pytest.raises(NotImplementedError):     # Pixelcoreg_Focalloss reads channels 0 and 1 only in the reference itself
        U.Pixelcoreg_Focalloss_twomodel()(z[:, :3].contiguous(), z[:, :3].contiguous(), t, 0.2, 0.5, dev)
    # the library's own guard: a class count outside 2 .. aide_seg_max_classes() is a negative code and launches nothing
    from aide_amd._lib import lib
    from aide_amd.ops import ptr, stream_ptr
    assert lib.aide_seg_max_classes() == 8
    for c in (1, 9):
        zc = z[:, :c].contiguous()
        part = torch.full((lib.aide_seg_loss_ws_bytes(2, 64) // 8,), -7.0, dtype=torch.float64, device=dev)
        out = torch.full((2, 8, 8), -7.0, device=dev)
        assert lib.aide_seg_stats(ptr(zc), c * 64, ptr(t), 64, None, c, 255, None, 0, None, 0, 2, 64, ptr(part), stream_ptr()) < 0
        assert lib.aide_kl_map(ptr(zc), c * 64, ptr(zc), c * 64, c, 2, 64, ptr(out), None, None, 0, None, 0, stream_ptr()) < 0
        torch.cuda.synchronize()
        assert bool((part == -7.0).all()) and bool((out == -7.0).all())
