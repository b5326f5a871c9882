"""Shared by test_loss_reference_host.py and test_gpu_loss_paths.py: the cases of the fused loss kernels (csrc/loss.hip), their
operands and a float64 reference written out from the math in the header comment of loss.hip and from oracle/losses.py.
Everything here is plain torch on the CPU; no library call and no golden file.

CASES              Case(n, h, w, c): every geometry crossed with every class count 2 .. 8, plus one batch-shaped geometry
                   (N = 260 > the 256 threads of the finalize kernels) for C = 2 and 5.  Which block split each HW lands on
                   follows from the library's own rule (aide_seg_loss_blocks); test_loss_reference_host.py asks the library and
                   fails when a required branch loses its case.
operands(case)     -> Operands: fp32 tensors seeded by the case's name.  Logits are randn * 3 with a per-image offset on the
                   class-1 plane (per-image losses apart), targets uniform in [0, C), image 0 carries an ignored stretch,
                   (3, 46, 50) an all-zero and an all-ignored image.
FORMS              the drop-in modules and their constructor keywords (the same for aide_amd.utils and for oracle)
reference(case, form) -> (value, input gradient) in float64; every input is upcast first and nothing rounds to fp32.  The
                   statistics-based forms share three backward passes per case (CE, I and P; the other statistics are
                   piecewise constant in the logits): their gradient is the chain rule through the eight statistics.
coteach_*          the two-network small-loss selection: operands for any batch size, and the three variants of
                   coteach_finalize_kernel in float64 (oracle/losses.py, oracle/steps.proposed_losses)
guarded buffers    from wgrad_cases (one NaN bit pattern around and inside a view)"""
import collections
import functools
import zlib

import torch

from wgrad_cases import LEAD, NAN_BITS, all_pattern, guarded, guards_intact   # noqa: F401  (used by test_gpu_loss_paths.py)

Case = collections.namedtuple('Case', 'n h w c')

# (N, H, W): HW = 1 (255 idle threads), 35 (less than a wavefront), 2300 (2 blocks, last stride partial),
# 4100 (3 blocks with unequal iteration counts), 131044 (grid capped at 64 blocks, 8 strides per thread, ragged tail, N = 1)
GEOMETRIES = ((3, 1, 1), (2, 5, 7), (3, 46, 50), (2, 50, 82), (1, 362, 362))
BATCH_GEOMETRY = (260, 4, 4)        # N > 256: the N-strided loops of the finalize kernels
CLASS_COUNTS = tuple(range(2, 9))
CASES = tuple(Case(n, h, w, c) for (n, h, w) in GEOMETRIES for c in CLASS_COUNTS) + \
    tuple(Case(*(BATCH_GEOMETRY + (c,))) for c in (2, 5))
EDGE_GEOMETRY = (3, 46, 50)         # image 1: all-zero target, image 2: every pixel ignored
ABI_CASES = tuple(Case(n, h, w, c) for (n, h, w) in ((3, 46, 50), (2, 50, 82)) for c in (2, 4, 7))
COTEACH_CLASSES = (2, 4, 7)
COTEACH_SPLITS = ((2, 1), (3, 2), (4, 2), (5, 4), (4, 4), (4, 5))      # (N, keep); (4, 4), (4, 5): D = 0 and keep > N
COTEACH_HW = (46, 50)
SATURATION_CASES = tuple(Case(2, 5, 7, c) for c in (2, 3, 8))
# statistics / finalize / backward in its three reductions, the two maps, the per-class Dice terms
SATURATION_FORMS = ('cemdice_mean', 'cemdice_sum', 'cemdice_image', 'ce_none', 'mse_wm_mean', 'mcdice_onehot_mean',
                    'mcdice_onehot_none')

IGNORE = 255
CEDICE = (0.7, 1.6)
RTOL, ATOL = 1e-4, 1e-9             # `close` of test_gpu_losses.py: max |got - ref| <= 1e-4 max |ref| + 1e-9
MIN_GAP = 1e-3                      # adjacent per-image losses further apart than this: the argsort is exact
P1_MARGIN = 1e-6                    # no p1 this close to the 0.5 threshold of the hard statistics
TOP2_MARGIN = 1e-6                  # labels are compared where the two largest probabilities are further apart
TOP2_CAP = 1e-3                     # at most this share of the pixels may be closer


def case_id(c):
    return '%dx%dx%d-c%d' % (c.n, c.h, c.w, c.c)


def class_weights(c):
    return tuple(torch.linspace(0.5, 2.0, c).tolist())


Operands = collections.namedtuple('Operands', 'z t class_w pseudo wmap')


def _seed(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _off_threshold(z):
    """move the class-1 logit of the (rare) pixels whose float64 p1 is within 1e-5 of 0.5 by 0.01, so that the fp32 and
    the float64 hard statistics count the same pixels"""
    p1 = torch.softmax(z.double(), 1)[:, 1]
    z[:, 1][(p1 - 0.5).abs() < 1e-5] += 0.01
    return z


def _logits(g, n, c, h, w, roll=0):
    z = torch.randn(n, c, h, w, generator=g) * 3
    if n > 1:
        z[:, 1] += torch.linspace(-1.5, 1.5, n).roll(roll).view(n, 1, 1)
    return _off_threshold(z)


def _pseudo(g, n, c, h, w):
    q = torch.softmax(torch.randn(n, c, h, w, generator=g), 1)
    return q, (1.0 - 4.0 * q[:, 0] * q[:, 1]).unsqueeze(1).contiguous()


def _targets(g, n, c, h, w):
    t = torch.randint(0, c, (n, h, w), generator=g)
    if w >= 5:
        t[0, 0, :5] = IGNORE
    if (n, h, w) == EDGE_GEOMETRY:
        t[1] = 0
        t[2] = IGNORE
    return t


@functools.lru_cache(maxsize=None)
def operands(case):
    n, h, w, c = case
    for draw in range(32):          # small images: draw again until the per-image losses are apart (a rule on the inputs)
        g = _seed('%s#%d' % (case_id(case), draw))
        z = _logits(g, n, c, h, w)
        t = _targets(g, n, c, h, w)
        q, wm = _pseudo(g, n, c, h, w)
        o = Operands(z, t, class_weights(c), q, wm)
        if n == 1 or n > 8 or min_gap(o) > 2 * MIN_GAP:
            return o
    raise AssertionError('no draw of %s separates the per-image losses' % case_id(case))


def min_gap(o):
    """the smallest distance between two per-image losses, over the vectors whose argsort is compared exactly: CE + Dice
    with the class weights, weighted CE alone, Dice alone (float64)"""
    hw = o.z.shape[2] * o.z.shape[3]
    st1, stw = statistics(o.z.double(), o.t), statistics(o.z.double(), o.t, o.class_w)
    gap = float('inf')
    for per in (per_image_loss(stw, hw, *CEDICE), per_image_loss(stw, hw, 1.0, 0.0), per_image_loss(st1, hw, 0.0, 1.0)):
        s = torch.sort(per).values
        if s.numel() > 1:
            gap = min(gap, (s[1:] - s[:-1]).min().item())
    return gap


def saturated(case):
    """logits of the case scaled so that differences between classes reach +-80"""
    z = operands(case).z
    zs = z * (80.0 / (z.max() - z.min()).item())
    zs[0, 0, 0, 0], zs[0, 1, 0, 0] = 40.0, -40.0            # the full +-80 in both directions, whatever the draw
    zs[0, 0, 0, 1], zs[0, 1, 0, 1] = -40.0, 40.0
    return zs.contiguous()


@functools.lru_cache(maxsize=None)
def ensemble_passes(case):
    """eight logit tensors of the case's shape (pseudo_label_ensemble takes the first K)"""
    n, h, w, c = case
    g = _seed(case_id(case) + '/passes')
    return tuple(torch.randn(n, c, h, w, generator=g) * 2 for _ in range(8))


def index_targets(t):
    """the targets without ignored pixels (class 0 there): what a one-hot encoding can hold"""
    return torch.where(t == IGNORE, torch.zeros_like(t), t)


def onehot(t, c):
    return torch.nn.functional.one_hot(index_targets(t), c).permute(0, 3, 1, 2).float().contiguous()


def prob_input(case):
    """DiceLoss on a probability input: the fp32 class-1 soft-max of the logits, [N, H, W], and its 0 / 1 target"""
    o = operands(case)
    return torch.softmax(o.z, 1)[:, 1].contiguous(), (index_targets(o.t) == 1).float()


def upstream(v):
    """the upstream gradient of a non-scalar loss: linspace(0.5, 1.5), as multiclass_cases.upstream"""
    return torch.linspace(0.5, 1.5, v.numel(), dtype=v.dtype).view(v.shape).to(v.device)


# ------------------------------------------------------------------------------------------- float64 reference
STAT_NAMES = ('CE', 'Wsum', 'I', 'P', 'T', 'M', 'hP', 'hI')       # the order of the kernels' statistics


def statistics(z, t, class_w=None, pseudo=None, wmap=None):
    """the eight per-image statistics of seg_stats_kernel, float64 [N] each (differentiable in z where they depend on it).
    z: float64 logits [N, C, H, W]"""
    n, c = z.shape[:2]
    cw = torch.ones(c, dtype=torch.float64) if class_w is None else torch.tensor(class_w, dtype=torch.float64)
    logp = torch.log_softmax(z, 1)
    p = torch.softmax(z, 1)
    valid = (t != IGNORE) & (t >= 0) & (t < c)
    tc = torch.where(valid, t, torch.zeros_like(t))
    wt = cw[tc] * valid.double()
    nll = -logp.gather(1, tc.unsqueeze(1)).squeeze(1)
    tf = t.double()                                  # the Dice terms read the index as a number, ignored pixels included
    p1 = p[:, 1]
    hard = (p1 >= 0.5).double()
    s = lambda x: x.reshape(n, -1).sum(1)
    st = dict(CE=s(wt * nll), Wsum=s(wt), I=s(p1 * tf), P=s(p1), T=s(tf), hP=s(hard), hI=s(hard * tf))
    if pseudo is not None:
        e2 = ((p - pseudo.double()) ** 2).sum(1)
        st['M'] = s(e2 if wmap is None else wmap.double().reshape(e2.shape) * e2)
    else:
        st['M'] = torch.zeros(n, dtype=torch.float64)
    return st


def dice_of(st, smooth):
    return 1.0 - (2.0 * st['I'] + smooth) / (st['P'] + st['T'] + smooth)


def per_image_loss(st, hw, w_ce, w_dice, smooth=1.0):
    return w_ce * st['CE'] / hw + w_dice * dice_of(st, smooth)


def reduce_loss(st, hw, w_ce, w_dice, smooth, reduction):
    """the three reductions of seg_finalize_kernel: 'mean' = w_ce sum CE / sum W + w_dice mean Dice, 'sum', 'image'"""
    if reduction == 'mean':
        return w_ce * (st['CE'].sum() / st['Wsum'].sum()) + w_dice * (dice_of(st, smooth).sum() / st['CE'].numel())
    if reduction == 'sum':
        return w_ce * st['CE'].sum() + w_dice * dice_of(st, smooth).sum()
    return per_image_loss(st, hw, w_ce, w_dice, smooth)


def hard_dice_sum(st):
    """Dice_fn: hard Dice summed over the batch; an empty target counts 1 when the prediction is empty too, else 0"""
    total = 0.0
    for hp, hi, tt in zip(st['hP'].tolist(), st['hI'].tolist(), st['T'].tolist()):
        total += (1.0 if hp == 0 else 0.0) if tt == 0 else 2.0 * hi / (hp + tt)
    return total


def label_reference(z):
    """-> (labels: first index of the largest float64 probability, sure: the two largest further apart than TOP2_MARGIN)"""
    p = torch.softmax(z.double(), 1)
    top = p.topk(2, dim=1).values
    return p.argmax(1), (top[:, 0] - top[:, 1]) > TOP2_MARGIN


@functools.lru_cache(maxsize=None)
def ensemble_mean(case, k):
    """float64 mean soft-max over the first k passes of the case"""
    return sum(torch.softmax(z.double(), 1) for z in ensemble_passes(case)[:k]) / float(k)


def pseudo_label_reference(passes, temperature, mean=None):
    """mean soft-max over the passes -> p^T / sum p^T -> 1 - 4 q0 q1, float64"""
    acc = sum(torch.softmax(z.double(), 1) for z in passes) / float(len(passes)) if mean is None else mean
    m = acc ** temperature
    q = m / m.sum(1, keepdim=True)
    return q, (1.0 - 4.0 * q[:, 0] * q[:, 1]).unsqueeze(1)


def _floats(w):
    return None if w is None else tuple(float(x) for x in w)


def statistics_form(name, kw, onehot_targets=False):
    """the drop-in modules that are a function of the eight statistics: module name and constructor keywords ->
    (class weights or None, w_ce, w_dice, smooth, reduction 'mean' | 'sum' | 'image'), or None for the other modules"""
    red = kw.get('reduction', 'mean')
    if name == 'CrossEntropyLoss2d' and red != 'none':
        return _floats(kw.get('weight')), 1.0, 0.0, 1.0, red
    if name in ('DiceLoss', 'Dice_Loss') or (name == 'MulticlassDiceLoss' and not onehot_targets):
        # class-1 Dice only; MulticlassDiceLoss ignores its class weights on index targets (utils/loss2d.py:105-106)
        return None, 0.0, 1.0, float(kw.get('smooth', 1.0)), 'image' if red == 'none' else red
    if name in ('CEMDiceLoss', 'CEMDiceLossImage', 'CEDiceLoss'):
        cd = _floats(kw.get('cediceweight')) or (1.0, 1.0)
        cw = _floats(kw.get('classweight' if name == 'CEDiceLoss' else 'ceclassweight'))
        return cw, cd[0], cd[1], 1.0, 'image' if name == 'CEMDiceLossImage' else red
    return None


def module_value(name, kw, z, t):
    """float64 value of the drop-in module name(**kw) on float64 logits z [N, C, H, W] and targets t (index [N, H, W], or
    one-hot [N, C, H, W]), written out from the math: the autograd graph to z is kept"""
    n, c, h, w = z.shape
    onehot_targets = t.dim() > 3
    if name == 'MulticlassMSELoss':                              # t: the pseudo label
        m = (torch.softmax(z, 1) - t.double()) ** 2
        red = kw.get('reduction', 'mean')
        return m if red == 'none' else m.mean() if red == 'mean' else m.sum()
    if onehot_targets and name != 'MulticlassDiceLoss':
        t, onehot_targets = t.argmax(1), False                   # utils/loss2d.py:11-12
    sf = statistics_form(name, kw, onehot_targets)
    if sf is not None:
        return reduce_loss(statistics(z, t, sf[0]), h * w, *sf[1:])
    red = kw.get('reduction', 'mean')
    cw = torch.ones(c, dtype=torch.float64) if kw.get('weight') is None else torch.tensor(_floats(kw['weight']),
                                                                                           dtype=torch.float64)
    if name == 'CrossEntropyLoss2d':                             # the reduction='none' map: w_t (lse - z_t), 0 where ignored
        tc = index_targets(t)
        return -torch.log_softmax(z, 1).gather(1, tc.unsqueeze(1)).squeeze(1) * cw[tc] * (t != IGNORE).double()
    assert name == 'MulticlassDiceLoss', name                    # one Dice term per class on one-hot targets, weighted
    smooth = float(kw.get('smooth', 1.0))
    p, oh = torch.softmax(z, 1).flatten(2), t.double().flatten(2)
    per = ((1.0 - (2.0 * (p * oh).sum(2) + smooth) / (p.sum(2) + oh.sum(2) + smooth)) * cw).sum(1)
    return per if red == 'none' else per.sum() / n if red == 'mean' else per.sum()


def _cw(o):
    return torch.tensor(o.class_w)


def _full(o):
    return dict(cediceweight=torch.tensor(CEDICE), ceclassweight=_cw(o), diceclassweight=_cw(o))


# form -> (module, constructor keywords from the case's operands, target kind): the same names and keywords build the
# module under test (aide_amd.utils), the fp32 oracle and, through module_value, the float64 reference
FORM_TABLE = collections.OrderedDict((
    ('ce_mean', ('CrossEntropyLoss2d', lambda o: dict(weight=_cw(o)), 'index')),
    ('ce_sum', ('CrossEntropyLoss2d', lambda o: dict(weight=_cw(o), reduction='sum'), 'index')),
    ('ce_none', ('CrossEntropyLoss2d', lambda o: dict(weight=_cw(o), reduction='none'), 'index')),
    ('dice_mean', ('DiceLoss', lambda o: dict(), 'index')),
    ('dice_sum', ('DiceLoss', lambda o: dict(smooth=0.5, reduction='sum'), 'index')),
    ('dice_none', ('DiceLoss', lambda o: dict(reduction='none'), 'index')),
    ('dice2_mean', ('Dice_Loss', lambda o: dict(smooth=0.25), 'index')),
    ('dice2_sum', ('Dice_Loss', lambda o: dict(reduction='sum'), 'index')),
    ('dice2_none', ('Dice_Loss', lambda o: dict(reduction='none'), 'index')),
    ('mcdice_index', ('MulticlassDiceLoss', lambda o: dict(weight=_cw(o)), 'index')),
    ('mcdice_onehot_mean', ('MulticlassDiceLoss', lambda o: dict(weight=_cw(o)), 'onehot')),
    ('mcdice_onehot_none', ('MulticlassDiceLoss', lambda o: dict(weight=_cw(o), smooth=0.5, reduction='none'), 'onehot')),
    ('cemdice_mean', ('CEMDiceLoss', _full, 'index')),
    ('cemdice_sum', ('CEMDiceLoss', lambda o: dict(_full(o), reduction='sum'), 'index')),
    ('cemdice_image', ('CEMDiceLossImage', _full, 'index')),
    ('cedice', ('CEDiceLoss', lambda o: dict(cediceweight=torch.tensor(CEDICE), classweight=_cw(o)), 'index')),
    ('mse_wm_mean', ('MulticlassMSELoss', lambda o: dict(reduction='none'), 'pseudo')),   # with the caller-side (wmap * m).mean()
))
FORMS = tuple(FORM_TABLE)
PROB_FORMS = collections.OrderedDict((('prob_dice_mean', dict()), ('prob_dice_none', dict(smooth=0.25, reduction='none')),
                                      ('prob_dice_sum', dict(reduction='sum'))))


def run_form(namespace, form, o):
    """value of the form through the modules of `namespace` (aide_amd.utils or oracle) on the operands o (on any device; o.z
    requires grad) -> (value, module)"""
    name, kw, kind = FORM_TABLE[form]
    m = getattr(namespace, name)(**kw(o))
    if kind == 'pseudo':
        return (o.wmap * m(o.z, o.pseudo)).mean(), m
    return m(o.z, onehot(o.t.cpu(), o.z.shape[1]).to(o.t.device) if kind == 'onehot' else o.t), m


def backward_of(v):
    (v * upstream(v)).sum().backward() if v.dim() else v.backward()


@functools.lru_cache(maxsize=None)
def base(case):
    """-> (statistics with unit class weights, with the case's class weights (both detached float64 [N]), and the gradients
    of the three differentiable ones: dict name -> [N, C, H, W]; CEw = CE with the class weights)"""
    o = operands(case)
    z = o.z.double().requires_grad_(True)
    st1 = statistics(z, o.t)
    stw = statistics(z, o.t, o.class_w)
    grads = {}
    for name, v in (('CE', st1['CE']), ('CEw', stw['CE']), ('I', st1['I']), ('P', st1['P'])):
        grads[name] = torch.autograd.grad(v.sum(), z, retain_graph=True)[0]      # images are independent: per-image rows
    det = lambda st: dict((k, v.detach()) for k, v in st.items())
    return det(st1), det(stw), grads


def _through_statistics(case, class_w, w_ce, w_dice, smooth, reduction):
    st1, stw, grads = base(case)
    assert class_w is None or class_w == operands(case).class_w
    st = st1 if class_w is None else stw
    leaves = dict((k, v.clone().requires_grad_(k in ('CE', 'I', 'P'))) for k, v in st.items())
    v = reduce_loss(leaves, case.h * case.w, w_ce, w_dice, smooth, reduction)
    out = (v * upstream(v)).sum() if v.dim() else v
    d = torch.autograd.grad(out, [leaves['CE'], leaves['I'], leaves['P']], allow_unused=True)
    g = torch.zeros_like(grads['P'])
    for dk, name in zip(d, ('CE' if class_w is None else 'CEw', 'I', 'P')):
        if dk is not None:
            g = g + dk.view(-1, 1, 1, 1) * grads[name]
    return v.detach(), g


def module_reference(name, kw, z, t, weight_map=None, up=upstream):
    """-> (value, gradient with respect to the logits) of module name(**kw) on any operands: float64, one plain autograd
    pass.  weight_map: the caller-side (weight_map * value).mean() of the consistency term; up: the upstream gradient of a
    non-scalar value"""
    z = z.double().requires_grad_(True)
    v = module_value(name, kw, z, t)
    if weight_map is not None:
        v = (weight_map.double() * v).mean()
    (v * up(v)).sum().backward() if v.dim() else v.backward()
    return v.detach(), z.grad


def direct(form, o):
    """the form on the operands o, without the shared statistics of `reference`"""
    name, kw, kind = FORM_TABLE[form]
    t = onehot(o.t, o.z.shape[1]) if kind == 'onehot' else o.pseudo if kind == 'pseudo' else o.t
    return module_reference(name, kw(o), o.z, t, o.wmap if kind == 'pseudo' else None)


@functools.lru_cache(maxsize=None)
def reference(case, form):
    """-> (value, gradient with respect to the logits) of a form on the case's operands, float64"""
    name, kw, kind = FORM_TABLE[form]
    sf = statistics_form(name, kw(operands(case)), kind == 'onehot')
    if sf is not None:
        return _through_statistics(case, *sf)
    return direct(form, operands(case))


@functools.lru_cache(maxsize=None)
def prob_reference(case, form):
    return prob_dice_reference(*(prob_input(case) + (PROB_FORMS[form],)))


def prob_dice_reference(x, t, kw, up=upstream):
    """DiceLoss(**kw) on a probability input x and its target, both flattened per image -> (value, gradient), float64"""
    smooth, red = float(kw.get('smooth', 1.0)), kw.get('reduction', 'mean')
    x = x.double().requires_grad_(True)
    n = t.shape[0]
    xf, tf = x.reshape(n, -1), t.double().reshape(n, -1)
    per = 1.0 - (2.0 * (xf * tf).sum(1) + smooth) / (xf.sum(1) + tf.sum(1) + smooth)
    v = per if red == 'none' else per.sum() / n if red == 'mean' else per.sum()
    (v * up(v)).sum().backward() if v.dim() else v.backward()
    return v.detach(), x.grad


def rel_err(got, ref):
    """max |got - ref| over (RTOL max |ref| + ATOL): at most 1 within the project's loss bound.  NaN only matches NaN."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    nan = torch.isnan(ref)
    if not torch.equal(torch.isnan(got), nan):
        return float('inf')
    if bool(nan.all()):
        return 0.0
    got, ref = got[~nan], ref[~nan]
    return (got - ref).abs().max().item() / (RTOL * ref.abs().max().item() + ATOL)


# ------------------------------------------------------------------------------------------- co-teaching selection
Coteach = collections.namedtuple('Coteach', 'z1 z2 t1 t2 q1 wm1 q2 wm2 class_w')


@functools.lru_cache(maxsize=None)
def coteach_operands(n, c):
    """two networks' logits on COTEACH_HW, two target sets, two pseudo labels with their weight maps.  Each image's logits
    are scaled by a factor of its own, 0.6 .. 1.4, rolled by one image for the second network: the cross-entropy against
    random targets grows with the scale, so the per-image losses are apart and the two rankings differ"""
    h, w = COTEACH_HW
    scale = torch.linspace(0.6, 1.4, n).view(n, 1, 1, 1)
    for draw in range(32):
        g = _seed('coteach-%d-c%d#%d' % (n, c, draw))
        z1, z2 = _off_threshold(_logits(g, n, c, h, w) * scale), _off_threshold(_logits(g, n, c, h, w, 1) * scale.roll(1, 0))
        t1, t2 = _targets(g, n, c, h, w), _targets(g, n, c, h, w)
        if n >= 3:                              # ordinary images only: the all-ignored image belongs to the table
            t1[2] = torch.randint(0, c, (h, w), generator=g)
            t2[2] = torch.randint(0, c, (h, w), generator=g)
        q1, wm1 = _pseudo(g, n, c, h, w)
        q2, wm2 = _pseudo(g, n, c, h, w)
        o = Coteach(z1, z2, t1, t2, q1, wm1, q2, wm2, class_weights(c))
        if coteach_min_gap(o) > 2 * MIN_GAP:
            return o
    raise AssertionError('no draw separates the per-image losses of %d images, %d classes' % (n, c))


def coteach_min_gap(o):
    """the smallest distance between two per-image losses of one network, over both networks, own and crossed targets (the
    proposed step scores net 1 against targets 2), with class weights and CEDICE and with neither"""
    hw = o.z1.shape[2] * o.z1.shape[3]
    gap = float('inf')
    for z, t in ((o.z1, o.t1), (o.z2, o.t2), (o.z1, o.t2), (o.z2, o.t1)):
        for cw, w_ce, w_dice in ((o.class_w,) + CEDICE, (None, 1.0, 1.0), (None, 0.7, 1.0)):
            s = torch.sort(per_image_loss(statistics(z.double(), t, cw), hw, w_ce, w_dice)).values
            gap = min(gap, (s[1:] - s[:-1]).min().item())
    return gap


def stable_argsort(v):
    """ascending, ties by index, NaN last (torch.sort / np.argsort)"""
    return torch.sort(v, stable=True).indices


def _mean(v):
    return v.sum() / v.numel() if v.numel() else v.sum() * float('nan')      # the mean of an empty set is NaN


def coteach_reference(z1, z2, t1, t2, variant, keep, w_ce, w_dice, class_w=None, smooth=1.0, rate=0.0, w_seg=1.0, w_cor=0.0,
                      q1=None, wm1=None, q2=None, wm2=None):
    """float64 form of coteach_finalize_kernel.  Net K is scored against t K / q K / wm K; it is trained on the images the
    OTHER net ranks as small-loss.  variant 0: the proposed inline step (oracle/steps.proposed_losses), 1: dropimage,
    2: weightimage (oracle/losses.py).  -> dict(loss1, loss2, grad1, grad2, per_image1, per_image2, argsort1, argsort2)"""
    hw = z1.shape[2] * z1.shape[3]
    n, c = z1.shape[:2]
    out, pers, zs = {}, [], []
    for z, t, q, wm in ((z1, t1, q1, wm1), (z2, t2, q2, wm2)):
        z = z.double().requires_grad_(True)
        st = statistics(z, t, class_w, q, wm)
        zs.append(z)
        pers.append((per_image_loss(st, hw, w_ce, w_dice, smooth), st['M']))
    order = [stable_argsort(p.detach()) for p, _ in pers]
    r = min(keep, n)
    for me in (0, 1):
        sel = order[1 - me]
        kept, dropped = sel[:r], sel[r:]
        per, m = pers[me]
        if variant == 0:
            loss = w_seg * (_mean(per[kept]) + (1.0 - rate) * _mean(per[dropped])) + \
                w_cor * rate * _mean(m[dropped]) / (c * hw)
        elif variant == 1:
            loss = _mean(per[kept])
        else:
            loss = _mean(per[kept]) + (0.1 * _mean(per[dropped]) if len(dropped) else 0.0)
        out['loss%d' % (me + 1)] = loss.detach()
        out['grad%d' % (me + 1)] = torch.autograd.grad(loss, zs[me])[0]
        out['per_image%d' % (me + 1)] = per.detach()
        out['argsort%d' % (me + 1)] = order[me]
    return out
