"""Float64 parity of the Spatial_Attention kernels (aide_amd/csrc/attention.hip: 1x1 conv, dilated 3x3 conv, BatchNorm2d(1) +
sigmoid gate, gate multiply, and their backward) and of the ConvTranspose2d(2, 2) kernels (aide_amd/csrc/convt.hip) on
every launch path of their extern "C" entries and on the layouts the engine hands them (-m gpu).  References, tables and
dispatch predicates: tests/attention_cases.py, validated on the host by tests/test_attention_reference_host.py, where the
kernel each row reaches is written down.  Each test id names that kernel.

Every tensor a kernel writes (outputs, stat, dw / db, dgamma / dbeta, d t4, the running statistics, and workspaces of
exactly the documented size) lives in a sentinel-filled allocation; after the call everything outside it must still hold
the sentinel.

Layout kinds (attention_cases.KINDS): dense; slice = read operands on the hi half, written operands on the lo half of a
2C-channel buffer (the concat buffers of the engine); pad4 = batch stride C H W + 4 (still the 16-byte kernels);
pad1 / pad2 = batch stride C H W + 1 / + 2 (the <1> kernels even at H W % 4 == 0).  N >= 2 wherever the stride matters.

Tolerances: 2e-5 of max |ref| for conv outputs / gradients, the gate output and the running statistics; 1e-4 for d t4,
dgamma, dbeta.  One-sum results (dgamma, dbeta, bias gradients, dw of the R = 1 conv) are measured on the rms scale of
their float64 terms (attention_cases.rms_err).

Exact identities asserted on top (torch.equal):
  * two launches into fresh buffers agree (no launch-order or uninitialised-memory dependence);
  * accumulating dgrad == base + overwriting dgrad added on the device: the kernel adds the loaded base LAST (one fp32 add);
  * sa_mul == gate[:, None] * y on the device (one fp32 multiply);
  * eval-mode stat == (running_mean, 1 / sqrtf(running_var + eps)), running statistics and counter untouched;
  * convT forward with bias == forward without + b[co] (the store adds the bias to the finished accumulator);
  * the <1> kernels == the <4> kernels for pw_fwd, the plain pw_dgrad, sa_mul and sa_mul_bwd (and with it d t4, dgamma,
    dbeta): both instantiations run the same per-element chain acc += w * x over c (r) in the same order, Vec<1> only drops
    lanes 1..3.  Not asserted for the gate + dout form of pw_dgrad (see test_pw_dgrad_one_operand_pad2);
  * empty weight-gradient splits of the transposed conv leave exact zeros in their slabs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_cases as A
from attention_cases import Layout as L

pytestmark = pytest.mark.gpu

ORDER = ('dense', 'slice', 'pad4', 'pad1', 'pad2')
NAN = float('nan')


def _sid(c):
    return 'x'.join(str(int(v)) for v in c)


def _small(dev, n, dtype=torch.float32, fill=None):
    """a guarded 1-D buffer of exactly n elements -> (flat, view)"""
    flat = torch.full((n + 2 * A.GUARD,), A.SENT, device=dev, dtype=dtype)
    v = flat[A.GUARD:A.GUARD + n]
    if fill is not None:
        v.fill_(fill)
    return flat, v


def _small_intact(flat, n):
    return bool((flat[:A.GUARD] == A.SENT).all()) and bool((flat[A.GUARD + n:] == A.SENT).all())


# ================================================================================================ 1x1 conv
def _pw_shapes(case):
    n, c, r, h, w = case
    return (n, c, h, w), (n, r, h, w), h * w


def _pw_fwd_target(case, kind):
    xs, ys, hw = _pw_shapes(case)
    return A.pw_fwd_kernel(hw, A.bs_of(A.KINDS[kind][0], xs), A.bs_of(A.KINDS[kind][1], ys))


def _pw_dgrad_target(case, kind):
    xs, ys, hw = _pw_shapes(case)
    return A.pw_dgrad_kernel(hw, A.bs_of(A.KINDS[kind][0], ys), A.bs_of(A.KINDS[kind][1], xs), A.bs_of(A.KINDS[kind][0], xs))


PW_REACH = {A.PW[0]: 'hw24', A.PW[1]: 'hw15', A.PW[2]: 'fwd-staging-loop-second-trip-r1', A.PW[3]: 'dgrad-staging-loop-second-trip'}
PW_FWD = [(c, k, _pw_fwd_target(c, k)) for c in A.PW for k in ORDER]
PW_DGRAD = [(c, k, _pw_dgrad_target(c, k)) for c in A.PW for k in ORDER]


def _pw_fwd(dev, d, kx, ky, what):
    """forward with and without bias on one layout pair, twice -> the result with bias"""
    from aide_amd import ops
    _, xv = L(kx, d['x'].shape).put(d['x'], dev)
    wd, bd = d['w'].to(dev), d['b'].to(dev)
    ly = L(ky, d['y'].shape)
    out = []
    for bias, ref in ((bd, d['y']), (None, d['y_nobias']), (bd, d['y'])):
        fy, yv = ly.blank(dev)
        ops.pwconv_fwd(xv, wd, bias, yv)
        A.assert_close(yv, ref, A.CONV_TOL, 'y (bias %s) %s' % (bias is not None, what))
        assert ly.intact(fy), 'forward wrote outside its planes ' + what
        out.append(yv.contiguous())
    assert torch.equal(out[0], out[2]), 'two launches differ ' + what
    return out[0]


@pytest.mark.parametrize('p', PW_FWD, ids=lambda p: '%s-%s-%s-%s' % (_sid(p[0]), PW_REACH[p[0]], p[1], p[2]))
def test_pw_fwd(dev, p):
    case, kind, target = p
    _pw_fwd(dev, A.pw_case(*case), A.KINDS[kind][0], A.KINDS[kind][1], '%s %s -> %s' % (case, kind, target))


def _pw_dgrad(dev, d, kt, kdx, kdout, what):
    """{plain, gate + dout} x {overwrite, accumulate onto the case's base} -> the four results"""
    from aide_amd import ops
    _, tv = L(kt, d['dt'].shape).put(d['dt'], dev)
    _, ov = L(kdout, d['dout'].shape).put(d['dout'], dev)
    wd, gd, based = d['w'].to(dev), d['gate'].to(dev), d['base'].to(dev)
    ld = L(kdx, d['x'].shape)
    res = {}
    for fused in (False, True):
        for acc in (False, True):
            w2 = '%s%s %s' % ('fused' if fused else 'plain', ' accumulate' if acc else '', what)
            fd, dv = ld.put(d['base'], dev) if acc else ld.blank(dev)
            ops.pwconv_dgrad(tv, wd, dv, gate=gd if fused else None, dout=ov if fused else None, accumulate=acc)
            A.assert_close(dv, A.pw_dgrad_ref(d, fused, acc), A.CONV_TOL, 'dx ' + w2)
            assert ld.intact(fd), 'dgrad wrote outside its planes ' + w2
            res[fused, acc] = dv.contiguous()
        assert torch.equal(res[fused, True], based + res[fused, False]), 'accumulate != base + overwrite ' + what
    fd, dv = ld.blank(dev)
    ops.pwconv_dgrad(tv, wd, dv, gate=gd, dout=ov)
    assert torch.equal(dv.contiguous(), res[True, False]), 'two launches differ ' + what
    return res


@pytest.mark.parametrize('p', PW_DGRAD, ids=lambda p: '%s-%s-%s-%s' % (_sid(p[0]), PW_REACH[p[0]], p[1], p[2]))
def test_pw_dgrad(dev, p):
    case, kind, target = p
    rd, wr = A.KINDS[kind]
    _pw_dgrad(dev, A.pw_case(*case), rd, wr, rd, '%s %s -> %s' % (case, kind, target))


@pytest.mark.parametrize('which', ['x', 'y'])
def test_pw_fwd_one_operand_pad2(dev, which):
    """x or y alone on pad2, the other dense, HW = 24 -> pw_fwd_kernel<1>; bit-equal to pw_fwd_kernel<4> on dense operands"""
    d = A.pw_case(*A.PW_PAD2)
    vec = _pw_fwd(dev, d, 'dense', 'dense', 'dense -> pw_fwd_kernel<4>')
    sc = _pw_fwd(dev, d, 'pad2' if which == 'x' else 'dense', 'pad2' if which == 'y' else 'dense',
                 'only %s on pad2 -> pw_fwd_kernel<1>' % which)
    assert torch.equal(sc, vec)


@pytest.mark.parametrize('which', ['dt', 'dx', 'dout'])
def test_pw_dgrad_one_operand_pad2(dev, which):
    """dt, dx or dout alone on pad2 -> pw_dgrad_kernel<1> (dout: in the gate + dout form only, the plain form ignores its
    stride and stays on <4>); the plain form bit-equal to pw_dgrad_kernel<4> on dense operands.  The gate + dout form is held
    to float64 only: its product gate * dout sits between the end of the FMA chain and the base add, and on MI355X the two
    instantiations are not bit-equal there (the build contracts with -ffp-contract=fast, which may fuse that product into
    either neighbour; the difference is printed)"""
    d = A.pw_case(*A.PW_PAD2)
    vec = _pw_dgrad(dev, d, 'dense', 'dense', 'dense', 'dense -> pw_dgrad_kernel<4>')
    kinds = ['pad2' if which == k else 'dense' for k in ('dt', 'dx', 'dout')]
    sc = _pw_dgrad(dev, d, kinds[0], kinds[1], kinds[2], 'only %s on pad2 -> pw_dgrad_kernel<1>' % which)
    for key in vec:
        if key[0]:
            print('fused %s: <1> against <4> max abs diff %.2e' % (key, float((sc[key] - vec[key]).abs().max())))
        else:
            assert torch.equal(sc[key], vec[key]), key


@pytest.mark.parametrize('with_db', [True, False], ids=['db', 'nodb'])
@pytest.mark.parametrize('kx', ['hi', 'dense'])
@pytest.mark.parametrize('case', A.PW, ids=lambda c: '%s-pw_wgrad_kernel' % _sid(c))
def test_pw_wgrad(dev, case, kx, with_db):
    """pw_wgrad_kernel: x on the hi half of a concat buffer (or dense), dt dense; db=None leaves the bias column unwritten"""
    from aide_amd import ops
    n, c, r, h, w = case
    d = A.pw_case(*case)
    _, xv = L(kx, d['x'].shape).put(d['x'], dev)
    tv = d['dt'].to(dev)
    res = []
    for _ in range(2):
        fw, dw = _small(dev, r * c)
        fb, db = _small(dev, r)
        ops.pwconv_wgrad(tv, xv, dw.view(r, c), db if with_db else None)
        if r == 1:
            A.assert_close_rms(dw.view(r, c), d['dw'], A.pw_dw_terms(d), A.CONV_TOL, 'dw (R = 1) %s' % (case,))
        else:
            A.assert_close(dw.view(r, c), d['dw'], A.CONV_TOL, 'dw %s' % (case,))
        if with_db:
            A.assert_close_rms(db, d['db'], A.pw_db_terms(d), A.CONV_TOL, 'db %s' % (case,))
        else:
            assert bool((db == A.SENT).all()), 'db=None was written'
        assert _small_intact(fw, r * c) and _small_intact(fb, r), 'wgrad wrote outside dw / db'
        res.append((dw.clone(), db.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ================================================================================================ dilated conv
DCONV_REACH = {A.DCONV[0]: 'cin-ne-cout', A.DCONV[1]: 'cin-ne-cout-centre-tap-only', A.DCONV[2]: 'dilation-1',
               A.DCONV[3]: 'staging-loop-second-trip', A.DCONV[4]: 'wide-plane'}


@pytest.mark.parametrize('case', A.DCONV, ids=lambda c: '%s-dconv_kernel-fwd+transposed-%s' % (_sid(c), DCONV_REACH[c]))
def test_dconv(dev, case):
    """dconv_kernel: forward with bias and with b=None, the transposed (dgrad) form, each twice"""
    from aide_amd import ops
    n, cin, cout, h, w, dil = case
    d = A.dconv_case(*case)
    xd, wd, bd, gd = d['x'].to(dev), d['w'].to(dev), d['b'].to(dev), d['dy'].to(dev)
    ly, lx = L('dense', d['y'].shape), L('dense', d['x'].shape)
    out = []
    for bias, ref in ((bd, d['y']), (None, d['y_nobias']), (bd, d['y'])):
        fy, yv = ly.blank(dev)
        ops.dconv_small(xd, wd, bias, yv, dil)
        A.assert_close(yv, ref, A.CONV_TOL, 'y (bias %s) %s' % (bias is not None, case))
        assert ly.intact(fy), 'forward wrote outside y'
        out.append(yv.clone())
    assert torch.equal(out[0], out[2])
    out = []
    for _ in range(2):
        fx, dv = lx.blank(dev)
        ops.dconv_small(gd, wd, None, dv, dil, transposed=True)
        A.assert_close(dv, d['dx'], A.CONV_TOL, 'dx (transposed form) %s' % (case,))
        assert lx.intact(fx), 'transposed form wrote outside dx'
        out.append(dv.clone())
    assert torch.equal(out[0], out[1])


@pytest.mark.parametrize('with_db', [True, False], ids=['db', 'nodb'])
@pytest.mark.parametrize('case', A.DCONV, ids=lambda c: '%s-dconv_wgrad_kernel' % _sid(c))
def test_dconv_wgrad(dev, case, with_db):
    from aide_amd import ops
    n, cin, cout, h, w, dil = case
    d = A.dconv_case(*case)
    xd, gd = d['x'].to(dev), d['dy'].to(dev)
    fw, dw = _small(dev, cout * cin * 9)
    fb, db = _small(dev, cout)
    ops.dconv_small_wgrad(gd, xd, dw.view(cout, cin, 3, 3), db if with_db else None, dil)
    A.assert_close(dw.view(cout, cin, 3, 3), d['dw'], A.CONV_TOL, 'dw %s' % (case,))
    if with_db:
        A.assert_close_rms(db, d['db'], A.dconv_db_terms(d), A.CONV_TOL, 'db %s' % (case,))
    else:
        assert bool((db == A.SENT).all()), 'db=None was written'
    assert _small_intact(fw, cout * cin * 9) and _small_intact(fb, cout), 'wgrad wrote outside dw / db'


@pytest.mark.parametrize('kind', ['hi', 'pad1'])
def test_dconv_refuses_strided_operands(dev, kind):
    """the dilated kernels index dense [N][C][H][W] tensors: a channel slice or a padded batch stride must raise (_dense),
    with nothing launched"""
    from aide_amd import ops
    case = A.DCONV[4]
    n, cin, cout, h, w, dil = case
    d = A.dconv_case(*case)
    wd, bd = d['w'].to(dev), d['b'].to(dev)
    _, xs = L(kind, d['x'].shape).put(d['x'], dev)
    fy, ys = L(kind, d['y'].shape).blank(dev)
    fdense, ydense = L('dense', d['y'].shape).blank(dev)
    dw, db = torch.full_like(wd, A.SENT), torch.full_like(bd, A.SENT)
    assert not xs.is_contiguous() and not ys.is_contiguous()
    with pytest.raises(RuntimeError):
        ops.dconv_small(xs, wd, bd, ydense, dil)
    with pytest.raises(RuntimeError):
        ops.dconv_small(d['x'].to(dev), wd, bd, ys, dil)
    with pytest.raises(RuntimeError):
        ops.dconv_small_wgrad(d['dy'].to(dev), xs, dw, db, dil)
    torch.cuda.synchronize()
    assert all(bool((t == A.SENT).all()) for t in (fy, fdense, dw, db))


# ================================================================================================ gate
class _BN(object):
    """what ops.sa_gate_fwd reads of a BatchNorm2d(1), every tensor in a guarded allocation"""

    def __init__(self, dev):
        self.eps, self.momentum, self.flats = A.EPS, A.MOMENTUM, []
        for name, val, dt in (('weight', A.GAMMA, torch.float32), ('bias', A.BETA, torch.float32),
                              ('running_mean', A.RM0, torch.float32), ('running_var', A.RV0, torch.float32),
                              ('num_batches_tracked', A.NBT0, torch.int64)):
            flat, v = _small(dev, 1, dt, fill=val)
            self.flats.append(flat)
            setattr(self, name, v)

    def intact(self):
        return all(_small_intact(f, 1) for f in self.flats)


def _gate_fwd(dev, t4, training, bn=None):
    """-> bn, gate [n,h,w], stat [2] (guarded; asserted intact)"""
    from aide_amd import ops
    bn = bn or _BN(dev)
    n, _, h, w = t4.shape
    fg, g = _small(dev, n * h * w)
    fs, st = _small(dev, 2)
    gate = g.view(n, h, w)
    ops.sa_gate_fwd(t4.to(dev), bn, training, st, gate)
    assert _small_intact(fg, n * h * w) and _small_intact(fs, 2) and bn.intact(), 'sa_gate_fwd wrote outside gate / stat / bn'
    return bn, gate, st


def _gate_targets(case, kind):
    n, c, h, w = case[:4]
    rd, wr = A.KINDS[kind]
    s = (n, c, h, w)
    return (A.sa_mul_kernel(h * w, A.bs_of(rd, s), A.bs_of(wr, s)), A.sa_mul_bwd_kernel(h * w, A.bs_of(wr, s), A.bs_of(rd, s)))


GATE_REACH = {A.GATE[0]: 'm240', A.GATE[1]: 'm30', A.GATE[2]: 'm1200-reduction-second-trip-offset-mean', A.GATE[3]: 'm16'}
GATE_FWD = [(c, k, _gate_targets(c, k)[0]) for c in A.GATE for k in ORDER]
GATE_BWD = [(c, k, _gate_targets(c, k)[1]) for c in A.GATE for k in ORDER]


def _mul(dev, d, gate, ky, kout, ref, what):
    from aide_amd import ops
    _, yv = L(ky, d['y'].shape).put(d['y'], dev)
    lo = L(kout, d['y'].shape)
    fo, ov = lo.blank(dev)
    ops.sa_mul(gate, yv, ov)
    A.assert_close(ov, ref, A.GATE_TOL, 'gate * y ' + what)
    assert lo.intact(fo), 'sa_mul wrote outside its planes ' + what
    assert torch.equal(ov, gate[:, None] * yv), 'sa_mul != gate * y on the device ' + what
    return ov.contiguous()


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('p', GATE_FWD, ids=lambda p: '%s-%s-%s-bn1_stats_kernel+sa_gate_kernel+%s' % (_sid(p[0][:4]), GATE_REACH[p[0]], p[1], p[2]))
def test_gate_fwd(dev, p, training):
    case, kind, target = p
    d = A.gate_case(*case)
    what = '%s %s %s -> %s' % (case, kind, 'train' if training else 'eval', target)
    bn, gate, stat = _gate_fwd(dev, d['t4'], training)
    A.assert_close(gate, d['gate'] if training else d['gate_eval'], A.GATE_TOL, 'gate ' + what)
    _mul(dev, d, gate, A.KINDS[kind][0], A.KINDS[kind][1], d['out'] if training else d['out_eval'], what)
    if training:
        A.assert_close(bn.running_mean, d['rm'], A.GATE_TOL, 'running mean ' + what)
        A.assert_close(bn.running_var, d['rv'], A.GATE_TOL, 'running var ' + what)
        assert int(bn.num_batches_tracked) == d['nbt']
    else:
        rm, rv = np.float32(A.RM0), np.float32(A.RV0)
        rstd = np.float32(1.0) / np.sqrt(np.float32(rv + np.float32(A.EPS)))
        assert stat.cpu().numpy().tolist() == [float(rm), float(rstd)], 'eval stat ' + what
        assert float(bn.running_mean) == float(rm) and float(bn.running_var) == float(rv)
        assert int(bn.num_batches_tracked) == A.NBT0
    bn2, gate2, stat2 = _gate_fwd(dev, d['t4'], training)
    assert torch.equal(gate2, gate) and torch.equal(stat2, stat) and torch.equal(bn2.running_var, bn.running_var)


def _gate_bwd(dev, d, gate, stat, bn, kdout, ky, what):
    """-> dt4, dgamma, dbeta with the workspace of exactly M floats + 16 bytes, NaN-filled"""
    from aide_amd import ops
    n, c, h, w = d['y'].shape
    m = n * h * w
    _, ov = L(kdout, d['dout'].shape).put(d['dout'], dev)
    _, yv = L(ky, d['y'].shape).put(d['y'], dev)
    fws, ws = _small(dev, m + 4, fill=NAN)
    ft, dt4 = _small(dev, m)
    fg, dgam = _small(dev, 1)
    fb, dbet = _small(dev, 1)
    ops.sa_gate_bwd(ov, yv, gate, d['t4'].to(dev), stat, bn.weight, dgam, dbet, dt4.view(n, 1, h, w), ws)
    e = (A.rel_err(dt4.view(n, 1, h, w), d['dt4']), A.rms_err(dgam, d['dgamma'], d['dgamma_terms']),
         A.rms_err(dbet, d['dbeta'], d['dbeta_terms']))
    print('gate bwd %s: d t4 %.2e dgamma %.2e dbeta %.2e' % ((what,) + e))
    assert max(e) <= A.GATE_BWD_TOL, 'd t4 / dgamma / dbeta %s of their scales > %.1e: %s' % (e, A.GATE_BWD_TOL, what)
    assert _small_intact(fws, m + 4), 'sa_gate_bwd wrote outside its M floats + 16 bytes workspace ' + what
    assert _small_intact(ft, m) and _small_intact(fg, 1) and _small_intact(fb, 1), 'sa_gate_bwd wrote outside dt4 / dgamma / dbeta'
    assert not bool(torch.isnan(ws).any()), 'the workspace is not fully written'
    return dt4.clone(), dgam.clone(), dbet.clone()


@pytest.mark.parametrize('p', GATE_BWD, ids=lambda p: '%s-%s-%s-%s+bn1_bwd_reduce_kernel+bn1_bwd_apply_kernel' % (_sid(p[0][:4]), GATE_REACH[p[0]], p[1], p[2]))
def test_gate_bwd(dev, p):
    """training-mode backward w.r.t. t4 / gamma / beta; y on the read layout, dout on the written one of the kind (two
    different halves of a concat buffer on `slice`, as view(src) / gview(dst) are)"""
    case, kind, target = p
    d = A.gate_case(*case)
    what = '%s %s -> %s' % (case, kind, target)
    bn, gate, stat = _gate_fwd(dev, d['t4'], True)
    r1 = _gate_bwd(dev, d, gate, stat, bn, A.KINDS[kind][1], A.KINDS[kind][0], what)
    r2 = _gate_bwd(dev, d, gate, stat, bn, A.KINDS[kind][1], A.KINDS[kind][0], what)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2)), 'two launches differ ' + what


@pytest.mark.parametrize('which', ['y', 'out'])
def test_sa_mul_one_operand_pad2(dev, which):
    """y or out alone on pad2, HW = 120 -> sa_mul_kernel<1>; bit-equal to sa_mul_kernel<4>"""
    d = A.gate_case(*A.GATE[0])
    _, gate, _ = _gate_fwd(dev, d['t4'], True)
    vec = _mul(dev, d, gate, 'dense', 'dense', d['out'], 'dense -> sa_mul_kernel<4>')
    sc = _mul(dev, d, gate, 'pad2' if which == 'y' else 'dense', 'pad2' if which == 'out' else 'dense', d['out'],
              'only %s on pad2 -> sa_mul_kernel<1>' % which)
    assert torch.equal(sc, vec)


@pytest.mark.parametrize('which', ['dout', 'y'])
def test_sa_gate_bwd_one_operand_pad2(dev, which):
    """dout or y alone on pad2, HW = 120 -> sa_mul_bwd_kernel<1>; d t4, dgamma, dbeta bit-equal to the sa_mul_bwd_kernel<4> run"""
    d = A.gate_case(*A.GATE[0])
    bn, gate, stat = _gate_fwd(dev, d['t4'], True)
    vec = _gate_bwd(dev, d, gate, stat, bn, 'dense', 'dense', 'dense -> sa_mul_bwd_kernel<4>')
    sc = _gate_bwd(dev, d, gate, stat, bn, 'pad2' if which == 'dout' else 'dense', 'pad2' if which == 'y' else 'dense',
                   'only %s on pad2 -> sa_mul_bwd_kernel<1>' % which)
    assert all(torch.equal(a, b) for a, b in zip(sc, vec))


def test_gate_per_group(dev):
    """the engine's grouped training step: sa_gate_fwd on t4[g*m:(g+1)*m] for 2 groups of one BatchNorm == two separate
    forwards on copies of the groups (gate, and the running statistics / counter after both), and the float64 reference of
    two consecutive BatchNorm steps"""
    from aide_amd import ops
    n, c, h, w, offset, seed = A.GATE[2]
    t4 = A.gate_inputs(4, c, h, w, offset, seed)[0]
    m = 2
    td = t4.to(dev)
    bn = _BN(dev)
    fg, g = _small(dev, 4 * h * w)
    fs, stat = _small(dev, 2)
    gate = g.view(4, h, w)
    for gi in range(2):
        ops.sa_gate_fwd(td[gi * m:(gi + 1) * m], bn, True, stat, gate[gi * m:(gi + 1) * m])
    assert _small_intact(fg, 4 * h * w) and _small_intact(fs, 2) and bn.intact()
    bn2 = _BN(dev)
    parts = [_gate_fwd(dev, t4[gi * m:(gi + 1) * m].clone(), True, bn2) for gi in range(2)]
    assert torch.equal(gate, torch.cat([p[1] for p in parts])) and torch.equal(stat, parts[1][2])
    assert torch.equal(bn.running_mean, bn2.running_mean) and torch.equal(bn.running_var, bn2.running_var)
    assert int(bn.num_batches_tracked) == int(bn2.num_batches_tracked) == A.NBT0 + 2
    rm, rv = torch.tensor([A.RM0], dtype=torch.float64), torch.tensor([A.RV0], dtype=torch.float64)
    gam, bet = torch.tensor([A.GAMMA], dtype=torch.float64), torch.tensor([A.BETA], dtype=torch.float64)
    ref = torch.cat([torch.sigmoid(F.batch_norm(t4[gi * m:(gi + 1) * m].double(), rm, rv, gam, bet, True, A.MOMENTUM, A.EPS))
                     for gi in range(2)])[:, 0]
    A.assert_close(gate, ref, A.GATE_TOL, 'grouped gate')
    A.assert_close(bn.running_mean, rm, A.GATE_TOL, 'running mean after two groups')
    A.assert_close(bn.running_var, rv, A.GATE_TOL, 'running var after two groups')


# ================================================================================================ grid wrap
# N H W / 4 = 1 310 720 > 4096 x 256: on dense operands the <4> kernels run their grid-stride loop twice; on pad1 the <1>
# kernels (and always dconv_kernel, sa_gate_kernel, bn1_bwd_apply_kernel: one item per pixel) run it five times.
WRAP_KINDS = ('dense', 'pad1')


def _wrap_id(entry):
    def f(kind):
        n, c, r, h, w = A.WRAP_PW
        s = (n, c, h, w)
        b = A.bs_of(kind, s)
        name = {'pw_fwd': A.pw_fwd_kernel(h * w, b, b), 'pw_dgrad': A.pw_dgrad_kernel(h * w, b, b, b),
                'gate': 'sa_gate_kernel+%s+%s+bn1_bwd_apply_kernel' % (A.sa_mul_kernel(h * w, b, b), A.sa_mul_bwd_kernel(h * w, b, b))}[entry]
        return '%s-%s-grid-wrap' % (kind, name)
    return f


@pytest.mark.parametrize('kind', WRAP_KINDS, ids=_wrap_id('pw_fwd'))
def test_wrap_pw_fwd(dev, kind):
    from aide_amd import ops
    n, c, r, h, w = A.WRAP_PW
    assert n * h * w // 4 > A.GRID_CAP
    d = A.pw_case(*A.WRAP_PW)
    _, xv = L(kind, d['x'].shape).put(d['x'], dev)
    ly = L(kind, d['y'].shape)
    fy, yv = ly.blank(dev)
    ops.pwconv_fwd(xv, d['w'].to(dev), d['b'].to(dev), yv)
    e = A.rel_err(yv, d['y'])
    print('wrap pw fwd %s: %.2e' % (kind, e))
    assert e <= A.CONV_TOL and ly.intact(fy)


@pytest.mark.parametrize('kind', WRAP_KINDS, ids=_wrap_id('pw_dgrad'))
def test_wrap_pw_dgrad(dev, kind):
    """the gate + dout form accumulating onto the case's base"""
    from aide_amd import ops
    d = A.pw_case(*A.WRAP_PW)
    _, tv = L(kind, d['dt'].shape).put(d['dt'], dev)
    _, ov = L(kind, d['dout'].shape).put(d['dout'], dev)
    ld = L(kind, d['x'].shape)
    fd, dv = ld.put(d['base'], dev)
    ops.pwconv_dgrad(tv, d['w'].to(dev), dv, gate=d['gate'].to(dev), dout=ov, accumulate=True)
    e = A.rel_err(dv, A.pw_dgrad_ref(d, True, True))
    print('wrap pw dgrad %s: %.2e' % (kind, e))
    assert e <= A.CONV_TOL and ld.intact(fd)


def test_wrap_dconv_kernel_fwd(dev):
    """dconv_kernel: N H W = 5 242 880 pixels per output channel, five trips of the grid-stride loop"""
    from aide_amd import ops
    n, cin, cout, h, w, dil = A.WRAP_DCONV
    assert n * h * w > 4 * A.GRID_CAP
    d = A.dconv_case(*A.WRAP_DCONV)
    ly = L('dense', d['y'].shape)
    fy, yv = ly.blank(dev)
    ops.dconv_small(d['x'].to(dev), d['w'].to(dev), d['b'].to(dev), yv, dil)
    e = A.rel_err(yv, d['y'])
    print('wrap dconv fwd: %.2e' % e)
    assert e <= A.CONV_TOL and ly.intact(fy)


@pytest.mark.parametrize('kind', WRAP_KINDS, ids=_wrap_id('gate'))
def test_wrap_gate(dev, kind):
    """sa_gate_fwd (every thread of bn1_stats_kernel sums 5120 offset-mean elements), sa_mul, sa_gate_bwd"""
    d = A.gate_case(*A.WRAP_GATE)
    bn, gate, stat = _gate_fwd(dev, d['t4'], True)
    A.assert_close(gate, d['gate'], A.GATE_TOL, 'gate')
    A.assert_close(bn.running_mean, d['rm'], A.GATE_TOL, 'running mean')
    A.assert_close(bn.running_var, d['rv'], A.GATE_TOL, 'running var')
    _mul(dev, d, gate, kind, kind, d['out'], 'wrap ' + kind)
    _gate_bwd(dev, d, gate, stat, bn, kind, kind, 'wrap ' + kind)


# ================================================================================================ transposed conv
CONVT_REACH = {A.CONVT[0]: 'image-boundary-in-k-chunk', A.CONVT[1]: 'all-tiles-partial-dgrad-k12', A.CONVT[2]: 'two-m-tiles',
               A.CONVT[3]: 'three-n-tiles-splits-capped-by-kmax', A.CONVT[4]: '126-empty-splits'}
CONVT_P = [(c, k) for c in A.CONVT for k in A.CONVT_KINDS]


@pytest.mark.parametrize('p', CONVT_P, ids=lambda p: '%s-%s-convt_fwd+convt_dgrad+convt_wgrad+slab_sum-%s'
                         % (_sid(p[0]), p[1], CONVT_REACH[p[0]]))
def test_convt(dev, p):
    """aide_convT2x2_fwd (with bias and b=None), _dgrad, _wgrad with the workspace of exactly aide_convT2x2_wgrad_ws_bytes,
    NaN-filled; x and dx on one layout, y and dy on the other"""
    from aide_amd import ops
    from aide_amd._lib import lib
    case, kind = p
    n, ci, co, h, w = case
    kx, ky = A.CONVT_KINDS[kind]
    d = A.convt_case(*case)
    what = '%s %s' % (case, kind)
    _, xv = L(kx, d['x'].shape).put(d['x'], dev)
    wd, bd = d['w'].to(dev), d['b'].to(dev)
    ly, lx = L(ky, d['y'].shape), L(kx, d['x'].shape)
    out = []
    for bias, ref in ((bd, d['y']), (None, d['y_nobias']), (bd, d['y'])):
        fy, yv = ly.blank(dev)
        ops.convT2x2_fwd(xv, wd, bias, yv)
        A.assert_close(yv, ref, A.CONV_TOL, 'y (bias %s) %s' % (bias is not None, what))
        assert ly.intact(fy), 'forward wrote outside its planes ' + what
        out.append(yv.contiguous())
    assert torch.equal(out[0], out[2]), 'two launches differ ' + what
    assert torch.equal(out[0], out[1] + bd.view(1, co, 1, 1)), 'forward with bias != forward without + b ' + what
    _, gv = ly.put(d['dy'], dev)
    out = []
    for _ in range(2):
        fd, dv = lx.blank(dev)
        ops.convT2x2_dgrad(gv, wd, dv)
        A.assert_close(dv, d['dx'], A.CONV_TOL, 'dx ' + what)
        assert lx.intact(fd), 'dgrad wrote outside its planes ' + what
        out.append(dv.contiguous())
    assert torch.equal(out[0], out[1])
    nws = lib.aide_convT2x2_wgrad_ws_bytes(n, ci, co, h, w) // 4
    splits, per, live = A.convt_splits(*case)
    assert nws == splits * ci * co * 4
    out = []
    for _ in range(2):
        fws, ws = _small(dev, nws, fill=NAN)
        fw, dw = _small(dev, ci * co * 4)
        ops.convT2x2_wgrad(xv, gv, dw.view(ci, co, 2, 2), ws=ws)
        A.assert_close(dw.view(ci, co, 2, 2), d['dw'], A.CONV_TOL, 'dw ' + what)
        assert _small_intact(fws, nws), 'wgrad wrote outside its workspace ' + what
        assert _small_intact(fw, ci * co * 4), 'wgrad wrote outside dw ' + what
        slabs = ws.view(splits, ci * co * 4)
        assert not bool(torch.isnan(slabs).any()), 'a slab element was left unwritten ' + what
        assert live == splits or float(slabs[live:].abs().max()) == 0.0, 'an empty split is not an exact zero slab ' + what
        out.append(dw.clone())
    assert torch.equal(out[0], out[1])
