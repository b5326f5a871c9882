"""-m gpu: the fused Adam (aide_amd.optim.Adam -> adam_kernel, head_adam.hip) against torch.optim.Adam run on the CPU in
float64 (foreach=False: the plain single-tensor loop), element by element.

Both sides see the same gradient sequence: fp32 gradients drawn from a seeded generator, independent of the parameters,
widened to float64 for the reference.  The draws cover decaying magnitudes with sign flips (v shrinks, so the amsgrad
max matters for many elements), exact zeros, elements around 1e-8 (comparable to eps) and magnitudes from 1e-6 to 1e3.
The smallest nonzero gradient is ~1e-11, so g*g and (1 - beta2)*g*g stay fp32-normal: no subnormal arithmetic is tested.

The C ABI takes fp32 hyperparameters: the kernel is Adam with lr, betas, eps and weight decay rounded to fp32, and the
reference gets the same rounded values.  (Without that, 1 - beta2 alone would differ: 1 - fp32(0.999) is 1.3e-5 away
from 1 - 0.999 in relative terms, a property of the fp32 interface and not an arithmetic error.)

Bounds are in units of fp32 rounding of the operands, so that cancellation cannot make a correct result look wrong:
  m, vmax, v    |err| <= K ulp32 of the sum of the magnitudes of the two terms of the moving average,
  p             |err| <= 1 ulp32(p) + C * |update|, |update| = lr / bc1 * (that same m term sum) / denom.
A teacher-forced step starts both sides from the device's fp32 state, so any error present on every step (a bias
correction one step off, a skipped block tail, a dropped weight decay) shows on the step it happens."""
import io
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# Calibrated on the unmodified kernel (MI355X) over every teacher-forced step of this module, worst observed value in
# brackets; each limit is at most twice that.  g' = g + weight_decay * p.  The free-running drift stayed within 0.23 of its
# summed bound.
K_M = 3.0          # ulps of b1|m| + (1-b1)|g'|                  [observed 1.78]
K_V = 4.0          # ulps of b2 v + (1-b2) g'^2 (v and vmax)      [observed 2.89]
C_P = 5e-7         # relative error of the update beyond 1 ulp(p) [observed 2.86e-7]
P_ULPS = 1.0
SIZES = [1, 3, 255, 256, 257, 1023, 0, 1024, 1025, 4097, 65537, 0]


def f32(x):
    return float(np.float32(x))


def ulp32(x):
    """fp32 spacing at |x| (float64 tensor); 2^-149 below the normal range."""
    e = torch.frexp(x.abs().clamp_min(2.0 ** -126)).exponent
    return torch.ldexp(torch.ones_like(x), e - 24)


class Grads(object):
    """Seeded fp32 gradient sequence for a list of shapes."""

    def __init__(self, shapes, seed, steps=200):
        self.shapes = [tuple(s) if isinstance(s, (tuple, list, torch.Size)) else (s,) for s in shapes]
        self.g = torch.Generator().manual_seed(seed)
        self.base, self.rate, self.sign = [], [], []
        for s in self.shapes:
            n = math.prod(s)
            i = torch.arange(n)
            base = 10.0 ** (torch.rand(n, generator=self.g, dtype=torch.float64) * 9 - 6)          # 1e-6 .. 1e3
            base[i % 89 == 1] = 10.0 ** (torch.rand(int((i % 89 == 1).sum()), generator=self.g,
                                                    dtype=torch.float64) - 8.5)                        # ~ eps
            base[i % 97 == 0] = 0.0                                                                     # always zero
            self.base.append(base)
            self.rate.append(torch.rand(n, generator=self.g, dtype=torch.float64) * (5.0 / steps))    # decay to e^-5
            self.sign.append(torch.where(torch.rand(n, generator=self.g) < 0.5, -1.0, 1.0).double())
        self.t = 0

    def __call__(self):
        out = []
        for s, base, rate, k in zip(self.shapes, self.base, self.rate, range(len(self.shapes))):
            n = base.numel()
            flip = torch.rand(n, generator=self.g) < 0.3
            self.sign[k] = torch.where(flip, -self.sign[k], self.sign[k])
            noise = 0.5 + torch.rand(n, generator=self.g, dtype=torch.float64)
            g = base * torch.exp(-rate * self.t) * noise * self.sign[k]
            g[torch.rand(n, generator=self.g) < 0.05] = 0.0                                            # zero this step
            out.append(g.float().reshape(s))
        self.t += 1
        return out


class Pair(object):
    """aide_amd.optim.Adam on device parameters next to torch.optim.Adam on float64 CPU copies.  Gradients live in
    persistent device buffers (the engine's arena does the same), so the steady state takes the fast path."""

    def __init__(self, dev, init, groups=None, **defaults):
        from aide_amd.optim import Adam
        groups = groups or [(list(range(len(init))), {})]
        self.p = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
        self.buf = [torch.zeros_like(p) for p in self.p]
        self.r = [torch.nn.Parameter(t.double().clone()) for t in init]
        self.opt = Adam([dict(params=[self.p[i] for i in idx], **o) for idx, o in groups], **defaults)
        self.ref = torch.optim.Adam([dict(params=[self.r[i] for i in idx], **o) for idx, o in groups],
                                    foreach=False, **defaults)
        self.group_of = {}
        for gi, (idx, _) in enumerate(groups):
            for i in idx:
                self.group_of[i] = gi

    def set_grads(self, gs, device=True):
        """device=False: the caller has put the gradients into the device buffers itself"""
        for p, b, r, g in zip(self.p, self.buf, self.r, gs):
            if g is None:
                p.grad, r.grad = None, None
            else:
                if device:
                    b.copy_(g)
                p.grad, r.grad = b, g.double()

    def sync_hyper(self):
        """the reference steps with the fp32-rounded hyperparameters the kernel receives"""
        for rg, g in zip(self.ref.param_groups, self.opt.param_groups):
            rg['lr'], rg['eps'], rg['weight_decay'] = f32(g['lr']), f32(g['eps']), f32(g['weight_decay'])
            rg['betas'] = (f32(g['betas'][0]), f32(g['betas'][1]))
            rg['amsgrad'] = bool(g['amsgrad'])

    def dev_state(self):
        """per parameter: (step, p, m, v, vmax) as float64 CPU tensors; step None if the parameter has no state"""
        out = []
        for p in self.p:
            st = self.opt.state.get(p, {})
            q = p.detach().cpu().double()
            if not st:
                out.append((None, q, None, None, None))
                continue
            vm = st.get('max_exp_avg_sq')
            out.append((int(st['step']), q, st['exp_avg'].cpu().double(), st['exp_avg_sq'].cpu().double(),
                        None if vm is None else vm.cpu().double()))
        return out

    def ref_state(self, clone=True):
        def c(t):
            return t.clone() if clone and t is not None else t
        out = []
        for r in self.r:
            st = self.ref.state.get(r, {})
            if not st:
                out.append((None, c(r.detach()), None, None, None))
                continue
            out.append((int(st['step']), c(r.detach()), c(st['exp_avg']), c(st['exp_avg_sq']),
                        c(st.get('max_exp_avg_sq'))))
        return out

    def force(self):
        """copy the device's fp32 state into the reference.  A group that turned amsgrad on over a state without
        max_exp_avg_sq gets aide's documented rule (vmax starts from v): the float64 restatement of optim.py's clone.
        Returns the device state it copied."""
        state = self.dev_state()
        for i, (r, s) in enumerate(zip(self.r, state)):
            step, q, m, v, vm = s
            with torch.no_grad():
                r.copy_(q)
            if step is None:
                self.ref.state.pop(r, None)
                continue
            st = dict(step=torch.tensor(float(step)), exp_avg=m.clone(), exp_avg_sq=v.clone())
            if vm is not None:
                st['max_exp_avg_sq'] = vm.clone()
            elif self.ref.param_groups[self.group_of[i]]['amsgrad']:
                st['max_exp_avg_sq'] = v.clone()
            self.ref.state[r] = st
        return state

    def hyper(self, i):
        g = self.ref.param_groups[self.group_of[i]]
        return g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'], g['amsgrad']


def step_errors(pre, got, ref, g, hyper):
    """worst error of one step of one tensor in the units of the module docstring: dict m, v, vmax (ulps), p (C).
    pre: the state both sides started from; got / ref: the device's / the reference's state after the step."""
    lr, b1, b2, eps, wd, amsgrad = hyper
    _, p0, m0, v0, vm0 = pre
    step, p1, m1, v1, vm1 = ref
    if p0.numel() == 0:
        return {}
    g = g.double().reshape(p0.shape)
    m0 = torch.zeros_like(p0) if m0 is None else m0
    v0 = torch.zeros_like(p0) if v0 is None else v0
    ga = g.abs() + wd * p0.abs()
    mterms = b1 * m0.abs() + (1 - b1) * ga
    out = dict(m=((got[2] - m1).abs() / ulp32(mterms)).max().item(),
               v=((got[3] - v1).abs() / ulp32(b2 * v0 + (1 - b2) * ga * ga)).max().item())
    if amsgrad:
        vterms = torch.maximum(b2 * v0 + (1 - b2) * ga * ga, vm0 if vm0 is not None else v0)
        out['vmax'] = ((got[4] - vm1).abs() / ulp32(vterms)).max().item()
    vhat = vm1 if amsgrad else v1
    upd = lr / (1 - b1 ** step) * mterms / (vhat.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    excess = ((got[1] - p1).abs() - P_ULPS * ulp32(p1)).clamp_min(0)
    out['p'] = torch.where(excess > 0, excess / upd, excess).max().item()          # (NaN stays NaN)
    return out


LIMITS = dict(m=K_M, v=K_V, vmax=K_V, p=C_P)


def check_step(errs, what):
    for k, e in errs.items():
        assert e <= LIMITS[k], '%s: %s error %.3g > %.3g' % (what, k, e, LIMITS[k])


def _same(x, y):
    if x is None or y is None or not torch.is_tensor(x):
        return x is y or x == y
    return torch.equal(x, y)


def forced_step(pair, gs, what='', device_grads=True):
    """one teacher-forced step: both sides start from the device state; every element of every tensor is checked, the
    step counts must agree, and a parameter without a gradient must not move"""
    pair.sync_hyper()
    pre = pair.force()
    pair.set_grads(gs, device_grads)
    pair.opt.step()
    pair.ref.step()
    got, ref = pair.dev_state(), pair.ref_state(clone=False)
    for i, (g, a, b, c) in enumerate(zip(gs, pre, got, ref)):
        tag = '%s tensor %d (%d elements)' % (what, i, a[1].numel())
        assert b[0] == c[0], '%s: step %s, torch %s' % (tag, b[0], c[0])
        if g is None:
            assert all(_same(x, y) for x, y in zip(a, b)), tag + ' changed without a gradient'
            continue
        check_step(step_errors(a, b, c, g, pair.hyper(i)), tag)
    return got


def free_run(pair, grads, steps, sched=None):
    """both sides run on their own; returns the per-parameter bound: the per-step bound summed over the steps, along the
    reference trajectory"""
    bound = [torch.zeros_like(r, dtype=torch.float64) for r in pair.r]
    for _ in range(steps):
        pair.sync_hyper()
        gs = grads()
        pre = pair.ref_state()
        pair.set_grads(gs)
        pair.opt.step()
        pair.ref.step()
        post = pair.ref_state()
        for i, (g, a, c) in enumerate(zip(gs, pre, post)):
            if g is None or a[1].numel() == 0:
                continue
            lr, b1, b2, eps, wd, amsgrad = pair.hyper(i)
            m0 = torch.zeros_like(a[1]) if a[2] is None else a[2]
            mterms = b1 * m0.abs() + (1 - b1) * (g.double().abs() + wd * a[1].abs())
            vhat = c[4] if amsgrad else c[3]
            upd = lr / (1 - b1 ** c[0]) * mterms / (vhat.sqrt() / math.sqrt(1 - b2 ** c[0]) + eps)
            bound[i] += P_ULPS * ulp32(c[1]) + C_P * upd
        if sched is not None:
            sched.step()
    return bound


def check_free(pair, bound, what):
    for i, (p, r, b) in enumerate(zip(pair.p, pair.r, bound)):
        err = (p.detach().cpu().double() - r.detach()).abs()
        worst = (err / b.clamp_min(1e-300)).max().item() if err.numel() else 0.0
        assert worst <= 1.0, '%s tensor %d: drift %.3g of the summed per-step bound' % (what, i, worst)


def init_params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes]


def dev_bits(pair):
    """every device tensor the optimizer owns, for bit-exact comparisons"""
    out = []
    for p in pair.p:
        st = pair.opt.state.get(p, {})
        out.append((p.detach().cpu(), int(st['step']) if st else None,
                    *[st[k].cpu() for k in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq') if k in st]))
    return out


def assert_bits_equal(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y) and x[1] == y[1], '%s tensor %d: state layout / step differ' % (what, i)
        for u, w in zip(x[:1] + x[2:], y[:1] + y[2:]):
            assert torch.equal(u, w), '%s tensor %d differs' % (what, i)


OPTIONS = [
    # amsgrad, weight_decay, betas, eps
    (True, 0.0, (0.9, 0.999), 1e-8),
    (False, 0.0, (0.9, 0.999), 1e-8),
    (True, 1e-2, (0.5, 0.9), 1e-6),
    (False, 1e-2, (0.9, 0.999), 1e-6),
    (True, 0.0, (0.5, 0.9), 1e-8),
]


@pytest.mark.parametrize('opts', OPTIONS, ids=lambda o: 'ams%d-wd%g-b%g,%g-eps%g' % (o[0], o[1], o[2][0], o[2][1], o[3]))
def test_teacher_forced_steps(dev, opts):
    """150 steps, each from the device state, over tensors that straddle the 1024-element blocks (two of them empty)"""
    amsgrad, wd, betas, eps = opts
    pair = Pair(dev, init_params(SIZES, 1), lr=1e-3, betas=betas, eps=eps, weight_decay=wd, amsgrad=amsgrad)
    grads = Grads(SIZES, 2, steps=150)
    for t in range(150):
        got = forced_step(pair, grads(), 'step %d' % (t + 1))
    assert [s[0] for s in got] == [150] * len(SIZES)
    if amsgrad:     # the gradient draw must exercise the max: vmax > v for a good share of the elements
        vm = torch.cat([s[4].flatten() for s in got])
        v = torch.cat([s[3].flatten() for s in got])
        assert (vm > v).double().mean().item() > 0.3


@pytest.mark.parametrize('opts', OPTIONS, ids=lambda o: 'ams%d-wd%g-b%g,%g-eps%g' % (o[0], o[1], o[2][0], o[2][1], o[3]))
def test_free_running_trajectory(dev, opts):
    """the same sequence with no resync: systematic drift would exceed the summed per-step bound"""
    amsgrad, wd, betas, eps = opts
    pair = Pair(dev, init_params(SIZES, 1), lr=1e-3, betas=betas, eps=eps, weight_decay=wd, amsgrad=amsgrad)
    bound = free_run(pair, Grads(SIZES, 2, steps=150), 150)
    check_free(pair, bound, 'free run')


@pytest.mark.parametrize('policy', ['StepLR', 'PolyLR'])
def test_param_groups_and_lr_schedulers(dev, policy):
    """two groups with their own lr / weight decay / betas / amsgrad in one optimizer; the lr changes every step"""
    from torch.optim.lr_scheduler import StepLR
    from aide_amd.utils import PolyLR
    shapes = [257, 3, 1025, 1024, 0, 4097, 1]
    groups = [([0, 2, 4, 6], dict(lr=1e-3)),
              ([1, 3, 5], dict(lr=3e-4, weight_decay=1e-2, betas=(0.5, 0.9), amsgrad=False))]
    pair = Pair(dev, init_params(shapes, 3), groups, amsgrad=True)
    shadow = torch.optim.Adam([dict(params=[torch.zeros(1, requires_grad=True)], lr=o['lr']) for _, o in groups])

    def sched(opt):
        return StepLR(opt, step_size=1, gamma=0.93) if policy == 'StepLR' else PolyLR(opt, max_epoch=40, power=0.9)
    s, s_shadow = sched(pair.opt), sched(shadow)
    grads = Grads(shapes, 4, steps=60)
    for t in range(60):
        forced_step(pair, grads(), 'step %d' % (t + 1))
        shadow.step()
        s.step()
        s_shadow.step()
        assert [g['lr'] for g in pair.opt.param_groups] == [g['lr'] for g in shadow.param_groups]
    assert len(set(g['lr'] for g in pair.opt.param_groups)) == 2
    pair2 = Pair(dev, init_params(shapes, 3), groups, amsgrad=True)
    bound = free_run(pair2, Grads(shapes, 4, steps=60), 60, sched=sched(pair2.opt))
    check_free(pair2, bound, policy + ' free run')


def test_many_small_tensors(dev):
    """~1000 tensors: the block_start binary search over a long table, empty tensors among them"""
    g = torch.Generator().manual_seed(5)
    sizes = torch.randint(0, 2600, (1000,), generator=g).tolist()
    for i in (0, 17, 500, 999):
        sizes[i] = 0
    for i, n in ((1, 1), (2, 1024), (3, 1025), (998, 1)):
        sizes[i] = n
    pair = Pair(dev, init_params(sizes, 6), lr=1e-3, amsgrad=True, weight_decay=1e-2)
    grads = Grads(sizes, 7, steps=12)
    for t in range(12):
        forced_step(pair, grads(), 'step %d' % (t + 1))


def test_fuseunet_parameter_list(dev):
    """the real parameter list of the flagship network, 1024->512 conv weights included"""
    from aide_amd.models_twomodalinputs import fuseunet
    torch.manual_seed(2)
    init = [p.detach().clone() for p in fuseunet(2).parameters()]
    assert any(tuple(p.shape) == (512, 1024, 3, 3) for p in init)
    pair = Pair(dev, init, lr=1e-4, amsgrad=True)
    grads = Grads([p.shape for p in init], 8, steps=3)
    for t in range(3):
        forced_step(pair, grads(), 'step %d' % (t + 1))


def test_missing_gradients_and_late_joiner(dev):
    """torch counts steps per parameter: one with no gradient on a step keeps its state, and one frozen for the first 40
    steps starts at step 1 when it joins (one launch per distinct step count)"""
    shapes = [1025, 257, 4097, 3, 1024, 0]
    pair = Pair(dev, init_params(shapes, 9), lr=1e-3, amsgrad=True)
    late = pair.p[4]
    late.requires_grad_(False)
    grads = Grads(shapes, 10, steps=100)
    for t in range(100):
        gs = grads()
        if t % 3 == 1:
            gs[1] = None
        if t in (5, 6, 7, 50):
            gs[0] = None
        if t < 40:
            gs[4] = None
        elif t == 40:
            late.requires_grad_(True)
        got = forced_step(pair, gs, 'step %d' % (t + 1))
    assert [s[0] for s in got] == [96, 67, 100, 100, 60, 100]


def test_noncontiguous_gradients_and_zero_grad_in_place(dev):
    """transposed-view gradients, and gradients zeroed in place and accumulated into (zero_grad(set_to_none=False))"""
    shapes = [(33, 65), (1, 1), (48, 40), (1025,)]
    pair = Pair(dev, init_params(shapes, 11), lr=1e-3, amsgrad=True)
    for k in (0, 2):                                 # transposed storage: the gradient is a non-contiguous view
        pair.buf[k] = torch.zeros(tuple(reversed(shapes[k])), device=dev).t()
        assert not pair.buf[k].is_contiguous()
    grads = Grads(shapes, 12, steps=30)
    for t in range(30):
        gs = grads()
        if t % 2:
            pair.opt.zero_grad(set_to_none=False)
            assert all(p.grad is b and float(b.abs().max()) == 0 for p, b in zip(pair.p, pair.buf))
            for b, g in zip(pair.buf, gs):
                b.add_(g.to(dev))
        forced_step(pair, gs, 'step %d' % (t + 1), device_grads=not t % 2)


def _run(dev, steps, slow=False):
    """30-step runs on the block-straddling sizes: the same gradients whatever `steps` is"""
    pair = Pair(dev, init_params(SIZES, 13), lr=1e-3, amsgrad=True)
    grads = Grads(SIZES, 14, steps=30)
    pair.fast_ids = []
    for t in range(steps):
        if slow:
            pair.opt._fast.clear()
        pair.set_grads(grads())
        pair.opt.step()
        pair.fast_ids.append(id(pair.opt._fast.get(0)))
    return pair


def test_fast_path_bit_identical_to_slow_path(dev):
    fast = _run(dev, 30)
    assert id(None) not in fast.fast_ids and len(set(fast.fast_ids[1:])) == 1, 'the steady state left the fast path'
    assert_bits_equal(dev_bits(fast), dev_bits(_run(dev, 30, slow=True)), 'fast path vs slow path')


def test_state_changed_between_steps(dev):
    """a replaced moment tensor, new betas / weight decay, a reset step count: the next step must use them, as torch
    does, although every gradient is where it was (the fast path's case)"""
    pair = Pair(dev, init_params(SIZES, 15), lr=1e-3, amsgrad=True)
    grads = Grads(SIZES, 16, steps=45)
    held = []
    for t in range(45):
        st = [pair.opt.state[p] for p in pair.p] if t else []
        if t == 10:             # a fresh first moment; the old tensor stays alive, so a stale write would land in it
            held = [(s['exp_avg'], s['exp_avg'].clone()) for s in st]
            for s in st:
                s['exp_avg'] = torch.zeros_like(s['exp_avg'])
        if t == 15:
            held += [(s[k], s[k].clone()) for s in st for k in ('exp_avg_sq', 'max_exp_avg_sq')]
            for s in st:
                s['exp_avg_sq'] = s['exp_avg_sq'] * 0.25
                s['max_exp_avg_sq'] = s['max_exp_avg_sq'] * 0.5
        if t == 20:
            pair.opt.param_groups[0]['betas'] = (0.8, 0.99)
            pair.opt.param_groups[0]['weight_decay'] = 1e-2
        if t == 25:
            st[3]['step'] = 0
        if t == 32:
            for s in st:
                s['step'] = 2
        forced_step(pair, grads(), 'step %d' % (t + 1))
        for old, snap in held:
            assert torch.equal(old, snap), 'step %d wrote to a replaced state tensor' % (t + 1)
    steps = [int(pair.opt.state[p]['step']) for p in pair.p]
    assert steps == [15] * len(SIZES)
    assert 0 in pair.opt._fast, 'the fast path did not resume once the state was consistent again'


def test_amsgrad_switched_on_mid_run(dev):
    """torch fails on the missing max_exp_avg_sq; aide's rule (optim.py) is vmax starting from v, restated in float64"""
    pair = Pair(dev, init_params(SIZES, 17), lr=1e-3, amsgrad=False)
    grads = Grads(SIZES, 18, steps=30)
    for t in range(30):
        if t == 12:
            pair.opt.param_groups[0]['amsgrad'] = True
            assert all('max_exp_avg_sq' not in pair.opt.state[p] for p in pair.p)
        forced_step(pair, grads(), 'step %d' % (t + 1))
    assert all('max_exp_avg_sq' in pair.opt.state[p] for p in pair.p)


def test_checkpoint_torch_to_aide(dev):
    """a torch.optim.Adam state_dict (tensor step) taken at step 20 and loaded into aide's Adam; the run goes on"""
    for amsgrad_before in (True, False):
        pair = Pair(dev, init_params(SIZES, 19), lr=1e-3, amsgrad=amsgrad_before)
        pair.sync_hyper()
        grads = Grads(SIZES, 20, steps=40)
        for _ in range(20):
            pair.set_grads(grads())
            pair.ref.step()
        sd = pair.ref.state_dict()
        assert torch.is_tensor(sd['state'][0]['step'])
        with torch.no_grad():
            for p, r in zip(pair.p, pair.r):
                p.copy_(r.float())
        pair.opt.load_state_dict(sd)
        pair.opt.param_groups[0]['amsgrad'] = True       # from a non-amsgrad run: vmax starts from v
        pair.ref.param_groups[0]['amsgrad'] = True
        for p, r in zip(pair.p, pair.r):
            st, rs = pair.opt.state[p], pair.ref.state[r]
            assert int(st['step']) == 20 and st['exp_avg'].device == p.device and st['exp_avg'].dtype == torch.float32
            assert torch.equal(st['exp_avg'].cpu(), rs['exp_avg'].float())
            assert torch.equal(st['exp_avg_sq'].cpu(), rs['exp_avg_sq'].float())
            assert ('max_exp_avg_sq' in st) == amsgrad_before
        for t in range(20):
            got = forced_step(pair, grads(), 'amsgrad %s, step %d' % (amsgrad_before, t + 21))
        assert [s[0] for s in got] == [40] * len(SIZES)


def test_checkpoint_aide_to_torch(dev):
    """aide's state_dict (int step, device fp32 tensors) loaded into torch.optim.Adam: both continue from it"""
    pair = Pair(dev, init_params(SIZES, 21), lr=1e-3, amsgrad=True)
    grads = Grads(SIZES, 22, steps=50)
    for _ in range(20):
        pair.set_grads(grads())
        pair.opt.step()
    pair.sync_hyper()
    with torch.no_grad():
        for p, r in zip(pair.p, pair.r):
            r.copy_(p.double())
    pair.ref.load_state_dict(pair.opt.state_dict())
    pair.sync_hyper()
    pre = pair.dev_state()
    for a, r in zip(pre, pair.r):
        rs = pair.ref.state[r]
        assert float(rs['step']) == 20.0 and rs['exp_avg'].dtype == torch.float64 and not rs['exp_avg'].is_cuda
        assert torch.equal(rs['exp_avg'], a[2]) and torch.equal(rs['max_exp_avg_sq'], a[4])
    gs = grads()                                      # the first step runs from the loaded state as it is
    pair.set_grads(gs)
    pair.opt.step()
    pair.ref.step()
    for i, (g, a, b, c) in enumerate(zip(gs, pre, pair.dev_state(), pair.ref_state())):
        assert b[0] == c[0] == 21
        check_step(step_errors(a, b, c, g, pair.hyper(i)), 'first step after the load, tensor %d' % i)
    check_free(pair, free_run(pair, grads, 29), 'after the load')


def test_checkpoint_aide_to_aide_and_determinism(dev):
    """two identical runs are bit-identical, and so is a run saved at step 15 and resumed in a new optimizer"""
    a = _run(dev, 30)
    assert_bits_equal(dev_bits(a), dev_bits(_run(dev, 30)), 'rerun')
    from aide_amd.optim import Adam
    b = _run(dev, 15)
    buf = io.BytesIO()
    torch.save(b.opt.state_dict(), buf)
    params = [torch.nn.Parameter(p.detach().clone()) for p in b.p]
    opt = Adam(params, lr=1e-3, amsgrad=True)
    buf.seek(0)
    opt.load_state_dict(torch.load(buf))
    b.p, b.buf, b.opt = params, [torch.zeros_like(p) for p in params], opt
    grads = Grads(SIZES, 14, steps=30)
    for _ in range(15):
        grads()
    for _ in range(15):
        b.set_grads(grads())
        b.opt.step()
    assert_bits_equal(dev_bits(a), dev_bits(b), 'resumed run')


def test_steady_state_one_launch_per_group(dev, monkeypatch):
    from aide_amd.optim import Adam
    launches = []
    real = Adam._launch

    def counted(self, *a, **k):
        launches.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(Adam, '_launch', counted)
    shapes = [257, 3, 1025, 1024, 0, 4097, 1]
    pair = Pair(dev, init_params(shapes, 23), [([0, 2, 4, 6], {}), ([1, 3, 5], dict(lr=3e-4, amsgrad=False))],
                lr=1e-3, amsgrad=True)
    grads = Grads(shapes, 24, steps=10)
    for t in range(10):
        pair.set_grads(grads())
        del launches[:]
        pair.opt.step()
        assert len(launches) == 2, 'step %d: %d launches for 2 groups' % (t + 1, len(launches))
        if t:
            assert set(pair.opt._fast) == {0, 1}


def test_all_empty_group_is_a_noop(dev):
    """a group whose tensors are all empty: torch counts the step and updates nothing; so must aide (the kernel rejects
    an empty grid)"""
    pair = Pair(dev, [torch.zeros(0), torch.zeros(0, 3)], lr=1e-3, amsgrad=True)
    for t in range(3):
        got = forced_step(pair, [torch.zeros(0), torch.zeros(0, 3)], 'step %d' % (t + 1))
    assert [s[0] for s in got] == [3, 3]
