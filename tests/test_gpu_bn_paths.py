"""BatchNorm kernels (csrc/bn.hip) on every launch path, layout and storage combination, against float64 (-m gpu).  Cases, references
and bounds: tests/bn_cases.py (validated on the host by tests/test_bn_reference_host.py).  Replaces nn.BatchNorm2d (train) + nn.ReLU
and their autograd backward (reference: models_twomodalinputs/netblocks.py:24-28, models_singlemodalinput/UNet.py:19-23).

Every row: forward, apply and backward with and without the ReLU; coefficients, running statistics and num_batches_tracked against the
float64 operator; the activation bit-identical between the training forward and bn_relu_apply and within ONE rounding of the
contract under the device's own coefficients; dz, dgamma, dbeta, dbias against the contract -- no comparison is conditional, the
contract's mask is the kernel's mask.  Every buffer is a view inside a sentinel-filled allocation that must stay intact.  The path
predictor is pinned to the library by its three predicates and by the channel epochs every launch leaves in the workspace.

Largest share of its bound, device (host emulation, test_bn_reference_host.py), over all tests of this file (printed with -s);
116 tests, 8 s on an MI355X:
    coefficients and running statistics vs the float64 operator      0.98  (0.97)
    a vs the contract (one rounding)                                 1.00  (1.00)
    dz elementwise vs the contract                                   0.92  (0.91)
    dgamma / dbeta                                                   0.99  (0.98)
    dbias                                                            0.21  (0.16)
    group activations under the reference coefficients 0.67, coefficients from conv-epilogue entries 0.85 (against the true statistics
    of z 0.70), eval fold 0.75
A correctly counted rounding is used up to its full half spacing by some element of a large tensor, so a share near 1 is what a bound
without slack looks like; the device and the host emulation agree in every group.

Mutation check (each change alone, failing tests of this file / of the BatchNorm tests that were there before): HW / V - 1 in
bn_train_apply_kernel 52 / 3; cur.n * (C * HW) for cur.n * z_bs in bn_bwd_reduce_kernel 15 / 0; the ReLU applied whatever `relu` says in
bn_fwd_coop_kernel 34 / 0; the unguarded n / (n - 1) 2 / 0; gi for g0 + gi in the table store of bn_finalize_groups_kernel 4 / 0; the
conv bias not added to the mean 6 / 0; >= 0 for > 0 in the mask of bn_bwd_coop_kernel 2 / 0.
"""
import types

import pytest
import torch

import bn_cases as B
from bn_cases import Layout as L

pytestmark = pytest.mark.gpu
SHARES = {}
NAN = float('nan')


def _note(group, value):
    SHARES[group] = max(SHARES.get(group, 0.0), value)
    return value


def _epochs(ws, c):
    """generations completed per channel: the first int64 of every channel's workspace block"""
    return ws.view(torch.int64)[::B.WS_STRIDE][:c].clone()


def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _dev(t, dev):
    return t.to(dev) if t is not None else None


def _written(view, what):
    assert not bool((view == B.SENT).any()), '%s: an element of the view was never written' % what
    assert not bool(torch.isnan(view.float()).any()), '%s: NaN' % what


def _run(dev, shape, kinds, storage, op, relu, ws=None):
    """forward, apply, backward of one case through the ops wrappers -> dict of device tensors; asserts the layouts and the epochs"""
    from aide_amd import ops
    n, c, h, w = shape
    lz, la, ld, lo = (L(k, shape) for k in kinds)
    sz, sa, sd, so = storage
    fz, z = lz.put(op['z'], dev, _dt(sz))
    fd, dA = ld.put(op['dA'], dev, _dt(sd))
    fa, a = la.blank(dev, _dt(sa))
    fa2, a2 = la.blank(dev, _dt(sa))
    fo, dz = lo.blank(dev, _dt(so))
    gamma, beta = _dev(op['gamma'], dev), _dev(op['beta'], dev)
    rm, rv = (_dev(op['rm0'], dev), _dev(op['rv0'], dev)) if op['rm0'] is not None else (None, None)
    nbt = torch.full((), B.NBT0, dtype=torch.int64, device=dev) if rm is not None else None
    st = [torch.full((c,), NAN, device=dev) for _ in range(4)]
    dg, db, dbias = (torch.full((c,), NAN, device=dev) for _ in range(3))
    ws = ops.bn_ws(c, dev) if ws is None else ws
    fwd = B.predict_fwd(shape, lz.bs, la.bs, sz, sa)
    bwd = B.predict_bwd(shape, ld.bs, lz.bs, lo.bs, sd, sz, so)
    e0 = _epochs(ws, c)
    ops.bn_train_fwd(z, a, gamma, beta, B.EPS, B.MOM, rm, rv, nbt, st[0], st[1], st[2], st[3], ws, relu)
    e1 = _epochs(ws, c)
    ops.bn_relu_apply(z, a2, st[2], st[3], relu)
    ops.bn_relu_bwd(dA, z, dz, st[0], st[1], st[2], st[3], dg, db, dbias, ws, relu)
    e2 = _epochs(ws, c)
    assert bool((e1 - e0 == B.epoch_step(fwd)).all()), ('forward epochs', fwd, (e1 - e0).tolist()[:4])
    assert bool((e2 - e1 == B.epoch_step(bwd)).all()), ('backward epochs', bwd, (e2 - e1).tolist()[:4])
    for lay, flat, what in ((lz, fz, 'z'), (la, fa, 'a'), (la, fa2, 'a (apply)'), (ld, fd, 'dA'), (lo, fo, 'dz')):
        assert lay.intact(flat), '%s: written outside the view' % what
    assert torch.equal(z.float().cpu(), op['z']) and torch.equal(dA.float().cpu(), op['dA'])
    for view, what in ((a, 'a'), (a2, 'a (apply)'), (dz, 'dz')):
        _written(view, what)
    assert torch.equal(a, a2), 'training forward and bn_relu_apply differ'
    return dict(z=z, dA=dA, a=a, dz=dz, mean=st[0], rstd=st[1], scale=st[2], shift=st[3], rm=rm, rv=rv, nbt=nbt, dgamma=dg,
                dbeta=db, dbias=dbias, fwd=fwd, bwd=bwd, ws=ws, storage=storage)


def _hold(out, op, relu, dev, what):
    """an outcome of _run against both references"""
    z, dA = out['z'].float(), out['dA'].float()
    fwd, bwd = out['fwd'], out['bwd']
    gamma, beta, rm0, rv0 = (_dev(op[k], dev) for k in ('gamma', 'beta', 'rm0', 'rv0'))
    r1 = B.ref_operator(z, gamma, beta, rm0, rv0, stats_only=True)
    sb = B.stat_bounds(r1, gamma, beta, rm0, rv0)
    for k, bound in sb.items():
        s = _note('coefficients', B.share(out[k], r1[k], bound))
        assert s <= 1, (what, k, s)
    if out['nbt'] is not None:
        assert int(out['nbt'].item()) == B.NBT0 + 1
    r2 = B.ref_contract(z, dA, out['mean'], out['rstd'], out['scale'], out['shift'], relu)
    ab = B.a_bound(z, r2['y'], out['scale'], out['shift'])
    if out['storage'][1]:
        assert B.inside_bf16(out['a'], r2['a'], ab), (what, 'a (bf16)')
    else:
        assert _note('a', B.share(out['a'], r2['a'], ab)) <= 1, (what, 'a')
    if relu and not out['storage'][1]:
        assert torch.equal(out['a'] > 0, r2['mask']), (what, 'mask')
    bb = B.bwd_bounds(r2, out['scale'])
    if out['storage'][3]:
        assert B.inside_bf16(out['dz'], r2['dz'], bb['dz']), (what, 'dz (bf16)')
    for k in ('dgamma', 'dbeta', 'dbias') if out['storage'][3] else ('dz', 'dgamma', 'dbeta', 'dbias'):
        s = _note('dz' if k == 'dz' else 'dbias' if k == 'dbias' else 'sums', B.share(out[k], r2[k], bb[k]))
        assert s <= 1, (what, k, s)
    c = z.shape[1]
    if c >= 4:                                   # dA of the last channel is zero: c0 == c1 == 0, every dz there is an exact zero
        assert float(out['dz'][:, c - 1].float().abs().max()) == 0.0 and float(out['dgamma'][c - 1]) == 0.0 \
            and float(out['dbeta'][c - 1]) == 0.0 and float(out['dbias'][c - 1]) == 0.0


def test_predictor_matches_library(dev):
    from aide_amd._lib import lib
    shapes = {r.shape for r in B.ROWS} | {s for s, _ in B.layout_sweep()} | {(m, c, h, w) for _, m, _, c, h, w, _, _ in B.GROUP_ROWS}
    shapes |= {(4, 64, 64, 64), (4, 128, 32, 32), (2, 64, 16, 16), (4, 32, 256, 256), (8, 2, 514, 514), (3, 24, 40, 48), (2, 8, 6, 8)}
    for n, c, h, w in sorted(shapes):
        assert lib.aide_bn_one_pass(n, c, h, w) == B.one_pass(n, c, h, w), (n, c, h, w)
        assert lib.aide_bn_two_pass(n, c, h, w) == B.two_pass(n, c, h, w), (n, c, h, w)
        assert lib.aide_bn_relu_bwd_pool_supported(n, c, h, w) == B.pool_supported(n, c, h, w), (n, c, h, w)
    assert lib.aide_bn_ws_bytes(5) == 5 * B.WS_STRIDE * 8


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('name', [r.name for r in B.ROWS])
def test_row(dev, name, relu):
    row = B.ROW[name]
    op = B.row_operands(row)
    out = _run(dev, row.shape, row.kinds, row.storage, op, relu)
    assert B.path_of(out['fwd']) == row.fwd and B.path_of(out['bwd']) == row.bwd
    _hold(out, op, relu, dev, name)
    print('shares so far:', {k: round(v, 3) for k, v in SHARES.items()})


@pytest.mark.parametrize('shape,kinds', B.layout_sweep())
def test_layouts(dev, shape, kinds):
    op = B.operands(shape)
    for relu in (True, False):
        _hold(_run(dev, shape, kinds, B.F4, op, relu), op, relu, dev, (shape, kinds))


@pytest.mark.parametrize('name', B.STORAGE_ROWS)
def test_storage_combinations(dev, name):
    """the 4 forward and 8 backward storage combinations: statistics and coefficient vectors bit-identical to the fp32 call on the
    widened tensors, outputs the fp32 outputs rounded to nearest even; the fp32 call itself is held to the references"""
    from aide_amd import ops
    row = B.ROW[name]
    shape, kinds = row.shape, row.kinds
    n, c, h, w = shape
    op = B.operands(shape, bf16=True)
    base = _run(dev, shape, kinds, B.F4, op, True)
    _hold(base, op, True, dev, name)
    vec = ('mean', 'rstd', 'scale', 'shift', 'rm', 'rv')
    lz, la, ld, lo = (L(k, shape) for k in kinds)
    for sz, sa in B.FWD_STORAGE:
        fz, z = lz.put(op['z'], dev, _dt(sz))
        fa, a = la.blank(dev, _dt(sa))
        rm, rv = op['rm0'].to(dev), op['rv0'].to(dev)
        nbt = torch.full((), B.NBT0, dtype=torch.int64, device=dev)
        st = [torch.full((c,), NAN, device=dev) for _ in range(4)]
        ops.bn_train_fwd(z, a, op['gamma'].to(dev), op['beta'].to(dev), B.EPS, B.MOM, rm, rv, nbt, st[0], st[1], st[2], st[3],
                         base['ws'], True)
        got = dict(zip(vec, st + [rm, rv]))
        for k in vec:
            assert torch.equal(got[k], base[k]), (name, 'forward', (sz, sa), k, float((got[k] - base[k]).abs().max()))
        assert torch.equal(a, base['a'].to(_dt(sa))), (name, 'a', (sz, sa))
        assert lz.intact(fz) and la.intact(fa) and int(nbt.item()) == B.NBT0 + 1
    for sd, sz, so in B.BWD_STORAGE:
        fz, z = lz.put(op['z'], dev, _dt(sz))
        fd, dA = ld.put(op['dA'], dev, _dt(sd))
        fo, dz = lo.blank(dev, _dt(so))
        outs = [torch.full((c,), NAN, device=dev) for _ in range(3)]
        ops.bn_relu_bwd(dA, z, dz, base['mean'], base['rstd'], base['scale'], base['shift'], outs[0], outs[1], outs[2], base['ws'], True)
        for k, x in zip(('dgamma', 'dbeta', 'dbias'), outs):
            assert torch.equal(x, base[k]), (name, 'backward', (sd, sz, so), k, float((x - base[k]).abs().max()))
        assert torch.equal(dz, base['dz'].to(_dt(so))), (name, 'dz', (sd, sz, so))
        assert lz.intact(fz) and ld.intact(fd) and lo.intact(fo)


def _bn_of(op, dev):
    """the module-shaped argument of the stacked-batch wrappers"""
    return types.SimpleNamespace(weight=_dev(op['gamma'], dev), bias=_dev(op['beta'], dev), eps=B.EPS, momentum=B.MOM,
                                 running_mean=op['rm0'].to(dev).clone(), running_var=op['rv0'].to(dev).clone(),
                                 num_batches_tracked=torch.full((), B.NBT0, dtype=torch.int64, device=dev))


def _hold_groups(a, z, st, bn, op, m, groups, dev, what, relu=True, stat_ref=None, terms=None):
    """per-group activations and the walk of the running statistics; st: the LAST group's coefficients.  stat_ref(gi) -> (reference
    dict, extra keyword arguments of stat_bounds) when the statistics are not those of z itself"""
    gamma, beta = bn.weight, bn.bias
    rm, rv = op['rm0'].to(dev).double(), op['rv0'].to(dev).double()
    brm, brv = torch.zeros_like(rm), torch.zeros_like(rv)
    for gi in range(groups):
        zg = z[gi * m:(gi + 1) * m].float()
        if stat_ref is None:
            r1, kw = B.ref_operator(zg, gamma, beta, rm, rv, stats_only=True), {}
        else:
            r1, kw = stat_ref(gi, rm, rv)
        sb = B.stat_bounds(r1, gamma, beta, rm, rv, **kw)
        rm, rv = r1['rm'], r1['rv']
        brm, brv = brm + sb['rm'], brv + sb['rv']
        if a is not None:
            # the group's own coefficients are not returned (but for the last group): the activation of every group is held to the
            # contract under the REFERENCE coefficients, whose distance from the device's is bounded by sb
            y = zg.double() * B._v(r1['scale']) + B._v(r1['shift'])
            lim = B.a_bound(zg, y, r1['scale'], r1['shift']) + zg.double().abs() * B._v(sb['scale']) + B._v(sb['shift'])
            ref = torch.relu(y) if relu else y
            assert _note('a (groups)', B.share(a[gi * m:(gi + 1) * m], ref, lim)) <= 1, (what, gi)
    for k, x in zip(('mean', 'rstd', 'scale', 'shift'), st):
        assert _note('coefficients', B.share(x, r1[k], sb[k])) <= 1, (what, k)
    assert _note('coefficients', B.share(bn.running_mean, rm, brm)) <= 1 and _note('coefficients', B.share(bn.running_var, rv, brv)) <= 1
    assert int(bn.num_batches_tracked.item()) == B.NBT0 + groups
    if a is not None:                            # the last group exactly: one rounding under the returned coefficients
        zg = z[(groups - 1) * m:].float()
        ref, y = B.ref_forward(zg, st[2], st[3], relu)
        assert _note('a', B.share(a[(groups - 1) * m:], ref, B.a_bound(zg, y, st[2], st[3]))) <= 1, what


@pytest.mark.parametrize('case', B.GROUP_ROWS, ids=[g[0] for g in B.GROUP_ROWS])
def test_groups(dev, case):
    from aide_amd import ops
    name, m, groups, c, h, w, kinds, path = case
    shape = (m * groups, c, h, w)
    op = B.operands(shape, seed=1)
    lz, la = L(kinds[0], shape), L(kinds[1], shape)
    plan = B.predict_fwd((m, c, h, w), lz.bs, la.bs, groups=groups)
    assert B.path_of(plan) == path
    for relu in (True, False):
        fz, z = lz.put(op['z'], dev)
        fa, a = la.blank(dev)
        bn = _bn_of(op, dev)
        st = [torch.full((c,), NAN, device=dev) for _ in range(4)]
        ws = ops.bn_ws(c, dev)
        ops.bn_train_fwd_groups(z, a, groups, bn, st[0], st[1], st[2], st[3], ws, relu)
        assert bool((_epochs(ws, c) == B.epoch_step(plan, groups)).all())
        assert lz.intact(fz) and la.intact(fa)
        _written(a, 'a')
        _hold_groups(a, z, st, bn, op, m, groups, dev, name, relu)


PARTS_SHAPE = (5, 8, 20, 20)


def _parts_ref(parts, first, nparts, n, cb, gamma, beta, rm, rv):
    """reference dict of statistics taken from parts, with the running statistics; tight: the kernel sums the same fp32 entries"""
    rp = B.ref_from_parts(parts, first, nparts, n, cb, gamma, beta)
    rp['rm'], rp['rv'] = B.running_update(rm, rv, rp['mean'], rp['var'], n)
    return rp, dict(terms=nparts, mean_pre=rp['mean_pre'])


@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('nparts', B.PARTS_N)
def test_parts(dev, nparts, bias):
    """aide_bn_train_fwd_parts_strided: statistics from conv-epilogue entries (NaN in the entries of the wider stride that belong to
    nobody) -- coefficients tight against the float64 sum of the same entries, and against the true statistics of z to what the
    entries' own rounding implies; the activation to one rounding"""
    from aide_amd import ops
    shape = PARTS_SHAPE
    n, c, h, w = shape
    op = B.operands(shape)
    cb = torch.linspace(-1.0, 1.0, c).to(dev) if bias else None
    count = n * h * w
    for kind in ('dense', 'hi', 'pad4'):
        lay = L(kind, shape)
        fz, z = lay.put(op['z'], dev)
        fa, a = lay.blank(dev)
        stride, first = nparts + 7, 3
        parts = torch.full((c, stride, 2), NAN, device=dev)
        parts[:, first:first + nparts] = B.make_parts(z, cb, nparts)
        gamma, beta, rm, rv = (op[k].to(dev) for k in ('gamma', 'beta', 'rm0', 'rv0'))
        nbt = torch.full((), B.NBT0, dtype=torch.int64, device=dev)
        st = [torch.full((c,), NAN, device=dev) for _ in range(4)]
        # (`first` offsets the pointer: channel k's entries start at k * stride + first)
        ops.bn_train_fwd_parts(z, a, parts, nparts, cb, gamma, beta, B.EPS, B.MOM, rm, rv, nbt, st[0], st[1], st[2], st[3], True,
                               first=first, stride=stride)
        got = dict(zip(('mean', 'rstd', 'scale', 'shift', 'rm', 'rv'), st + [rm, rv]))
        rp, kw = _parts_ref(parts, first, nparts, count, cb, gamma, beta, op['rm0'].to(dev), op['rv0'].to(dev))
        sb = B.stat_bounds(rp, gamma, beta, op['rm0'].to(dev), op['rv0'].to(dev), **kw)
        for k, bound in sb.items():
            assert _note('coefficients (parts)', B.share(got[k], rp[k], bound)) <= 1, (kind, k)
        r1 = B.ref_operator(z, gamma, beta, op['rm0'].to(dev), op['rv0'].to(dev), stats_only=True)
        dm = B.U * rp['P1']
        r1 = dict(r1, A1=rp['A1'], A2=rp['A2'])          # (the magnitudes that were summed: those of z - conv_bias)
        sb = B.stat_bounds(r1, gamma, beta, op['rm0'].to(dev), op['rv0'].to(dev), terms=nparts, mean_pre=rp['mean_pre'], dm_extra=dm,
                           dvar_extra=B.U * rp['A2'] + 2 * rp['mean_pre'].abs() * dm)
        for k, bound in sb.items():
            assert _note('coefficients (parts, vs z)', B.share(got[k], r1[k], bound)) <= 1, (kind, k)
        ref, y = B.ref_forward(z, st[2], st[3])
        assert _note('a', B.share(a, ref, B.a_bound(z, y, st[2], st[3]))) <= 1
        assert lay.intact(fz) and lay.intact(fa) and int(nbt.item()) == B.NBT0 + 1
        _written(a, 'a')
        a2 = torch.empty_like(a)
        ops.bn_relu_apply(z, a2, st[2], st[3], True)
        assert torch.equal(a, a2)


def test_parts_through_groups(dev):
    """`parts` through aide_bn_train_fwd_groups: group g's entries at g * nparts of a wider stride"""
    from aide_amd import ops
    m, groups, c, h, w, nparts = 2, 3, 6, 8, 10, 5
    shape = (m * groups, c, h, w)
    op = B.operands(shape, seed=2)
    z = op['z'].to(dev)
    cb = torch.linspace(0.5, -0.5, c).to(dev)
    stride = nparts * groups + 4
    parts = B.make_parts(z, cb, nparts, groups, stride)
    assert bool(torch.isnan(parts[:, nparts * groups:]).all())
    for relu in (True, False):
        bn = _bn_of(op, dev)
        st = [torch.full((c,), NAN, device=dev) for _ in range(4)]
        a = torch.full_like(z, B.SENT)
        ops.bn_train_fwd_groups(z, a, groups, bn, st[0], st[1], st[2], st[3], None, relu, parts=parts, nparts=nparts,
                                parts_stride=stride, conv_bias=cb)
        _written(a, 'a')
        _hold_groups(a, z, st, bn, op, m, groups, dev, 'parts groups', relu,
                     stat_ref=lambda gi, rm, rv: _parts_ref(parts, gi * nparts, nparts, m * h * w, cb, bn.weight, bn.bias, rm, rv))


@pytest.mark.parametrize('tab_c0', [0, 5])
@pytest.mark.parametrize('groups', B.FINALIZE_GROUPS)
def test_finalize_groups(dev, groups, tab_c0):
    """aide_bn_finalize_groups: the per-group (scale, shift) table inside a wider sentinel-filled table (the second trip of the 32-group
    loop at 33 and 40 groups), running statistics after `groups` sequential updates, nbt, the last group's coefficients"""
    from aide_amd import ops
    m, c, h, w, nparts = 2, 6, 4, 4, 3
    shape = (m * groups, c, h, w)
    op = B.operands(shape, seed=3)
    z = op['z'].to(dev)
    for cb in (torch.linspace(-0.7, 0.9, c).to(dev), None):
        stride = nparts * groups + 2
        parts = B.make_parts(z, cb, nparts, groups, stride)
        bn = _bn_of(op, dev)
        st = [torch.full((c,), NAN, device=dev) for _ in range(4)]
        tab_c = tab_c0 + c + 3
        tab = torch.full((groups, tab_c, 2), B.SENT, device=dev)
        ops.bn_finalize_groups(m, groups, c, h, w, bn, parts, nparts, stride, cb, st[0], st[1], st[2], st[3], tab, tab_c0)
        outside = torch.ones(tab_c, dtype=torch.bool, device=dev)
        outside[tab_c0:tab_c0 + c] = False
        assert bool((tab[:, outside] == B.SENT).all()), 'table written outside [tab_c0, tab_c0 + C)'
        refs = {}

        def stat_ref(gi, rm, rv):
            refs[gi] = _parts_ref(parts, gi * nparts, nparts, m * h * w, cb, bn.weight, bn.bias, rm, rv)
            return refs[gi]
        _hold_groups(None, z, st, bn, op, m, groups, dev, 'finalize', stat_ref=stat_ref)
        for gi in range(groups):
            rp, kw = refs[gi]
            sb = B.stat_bounds(rp, bn.weight, bn.bias, None, None, **kw)
            assert _note('coefficients (parts)', B.share(tab[gi, tab_c0:tab_c0 + c, 0], rp['scale'], sb['scale'])) <= 1, gi
            assert _note('coefficients (parts)', B.share(tab[gi, tab_c0:tab_c0 + c, 1], rp['shift'], sb['shift'])) <= 1, gi
        assert torch.equal(tab[groups - 1, tab_c0:tab_c0 + c, 0], st[2]) and torch.equal(tab[groups - 1, tab_c0:tab_c0 + c, 1], st[3])


@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('affine', ['both', 'no_gamma', 'no_beta'])
def test_eval_fold(dev, affine, bias):
    from aide_amd import ops
    c = 70                                       # two workgroups of 64, the second ragged
    g = torch.Generator().manual_seed(11)
    gamma = None if affine == 'no_gamma' else (torch.rand(c, generator=g) - 0.5).to(dev) * 3
    beta = None if affine == 'no_beta' else torch.randn(c, generator=g).to(dev)
    rm, rv = torch.randn(c, generator=g).to(dev), (torch.rand(c, generator=g) * 4).to(dev)
    rv[3] = 0.0
    cb = torch.randn(c, generator=g).to(dev) if bias else None
    bn = types.SimpleNamespace(weight=gamma, bias=beta, running_mean=rm, running_var=rv, eps=B.EPS)
    out = torch.full((3, c + 2), B.SENT, device=dev)
    ops.bn_eval_fold(bn, cb, out[0, :c], out[1, :c], out[2, :c])
    assert bool((out[:, c:] == B.SENT).all())
    refs, bounds = B.eval_fold_ref(gamma, beta, rm, rv, cb)
    for k in range(3):
        assert _note('eval fold', B.share(out[k, :c], refs[k], bounds[k])) <= 1, k


@pytest.mark.parametrize('shape,tag,what', B.STRESS)
def test_stress(dev, shape, tag, what):
    """a constant channel (var = 0 or a rounding residue of either sign: the `var < 0` clamp), |mean| / std = 1e3, null gamma / beta,
    null running statistics with a null num_batches_tracked, a channel whose pre-activations are all exactly 0 (masked off: `> 0`)"""
    op = B.stress_operands(shape, what)
    for relu in (True, False):
        out = _run(dev, shape, B.D4, B.F4, op, relu)
        assert out['fwd'].form == ('one-pass' if tag == 'op' else 'two-pass')
        _hold(out, op, relu, dev, (tag, what))


def test_workspace_reuse(dev):
    """one zero-filled workspace of the largest C carries a one-pass S > 1 row, a two-pass row, a one-pass row with another C and S, a
    grouped row, then the first again: every result equals the result on a fresh workspace bit for bit, the epochs advance by exactly
    the predicted amounts (asserted inside _run) -- stale entries of earlier launches never match"""
    from aide_amd import ops
    seq = ['v4_s2', 'tp_v1_plane', 'v4_by_stride', 'groups', 'v4_s2']
    ws = ops.bn_ws(8, dev)
    keys = ('a', 'dz', 'mean', 'rstd', 'scale', 'shift', 'rm', 'rv', 'dgamma', 'dbeta', 'dbias')
    _, m, groups, c, h, w, _, _ = B.GROUP_ROWS[1]
    for name in seq:
        if name == 'groups':
            op = B.operands((m * groups, c, h, w), seed=1)
            z = op['z'].to(dev)
            res = []
            for w_ in (ops.bn_ws(c, dev), ws):
                e0 = _epochs(w_, 8)
                bn = _bn_of(op, dev)
                st = [torch.full((c,), NAN, device=dev) for _ in range(4)]
                a = torch.empty_like(z)
                ops.bn_train_fwd_groups(z, a, groups, bn, st[0], st[1], st[2], st[3], w_)
                step = _epochs(w_, 8) - e0
                assert bool((step[:c] == groups).all()) and bool((step[c:] == 0).all())
                res.append([a, bn.running_mean, bn.running_var] + st)
            for x, y in zip(*res):
                assert torch.equal(x, y)
            continue
        row = B.ROW[name]
        op = B.row_operands(row)
        fresh = _run(dev, row.shape, row.kinds, row.storage, op, True)
        used = _run(dev, row.shape, row.kinds, row.storage, op, True, ws=ws)
        for k in keys:
            assert torch.equal(fresh[k], used[k]), (name, k)
    assert _epochs(ws, 8).tolist() == [2 + 0 + 2 + 3 + 2] * 6 + [2 + 0 + 0 + 3 + 2] * 2


def _refused(call):
    with pytest.raises(RuntimeError, match='bad argument'):
        call()
    torch.cuda.synchronize()


def test_guards(dev):
    """every argument rule of the launchers returns its error code and writes nothing"""
    from aide_amd import ops
    shape = (2, 4, 3, 2)
    n, c, h, w = shape
    op = B.operands(shape)
    z, dA = op['z'].to(dev), op['dA'].to(dev)
    outs = [torch.full(shape, B.SENT, device=dev) for _ in range(2)]
    vecs = [torch.full((c,), B.SENT, device=dev) for _ in range(12)]
    gamma, beta = op['gamma'].to(dev), op['beta'].to(dev)
    bn = _bn_of(op, dev)
    ws = ops.bn_ws(c, dev)
    st = vecs[:4]
    _refused(lambda: ops.bn_train_fwd(z, outs[0], gamma, beta, B.EPS, B.MOM, vecs[4], vecs[5], None, st[0], st[1], st[2], st[3], None))
    _refused(lambda: ops.bn_relu_bwd(dA, z, outs[1], st[0], st[1], st[2], st[3], vecs[6], vecs[7], vecs[8], None))
    # slabs need planes that are a multiple of 4 values
    slabs = torch.zeros((2,) + shape, device=dev)
    _refused(lambda: ops.bn_train_fwd_slabs(ops.ptr(slabs), 2, slabs[0].numel(), None, outs[0], outs[1], gamma, beta, B.EPS, B.MOM,
                                            vecs[4], vecs[5], None, st[0], st[1], st[2], st[3], ws))
    _refused(lambda: ops.bn_train_fwd_groups(z, outs[0], 1, bn, st[0], st[1], st[2], st[3], None))
    # the conv-epilogue form: a stride below nparts * groups, a plane that is not a multiple of 4
    parts = torch.zeros(c, 8, 2, device=dev)
    _refused(lambda: ops.bn_train_fwd_parts(z, outs[0], parts, 2, None, gamma, beta, B.EPS, B.MOM, vecs[4], vecs[5], None, st[0], st[1],
                                            st[2], st[3]))
    s2 = (2, 4, 4, 2)
    z2, a2 = torch.zeros(s2, device=dev), torch.full(s2, B.SENT, device=dev)
    _refused(lambda: ops.bn_train_fwd_parts(z2, a2, parts, 4, None, gamma, beta, B.EPS, B.MOM, vecs[4], vecs[5], None, st[0], st[1],
                                            st[2], st[3], stride=3))
    _refused(lambda: ops.bn_train_fwd_groups(z2, a2, 2, bn, st[0], st[1], st[2], st[3], None, parts=parts, nparts=4, parts_stride=7))
    tab = torch.full((2, c + 1, 2), B.SENT, device=dev)
    _refused(lambda: ops.bn_finalize_groups(1, 2, c, 4, 2, bn, parts, 4, 8, None, st[0], st[1], st[2], st[3], tab, 2))
    _refused(lambda: ops.bn_finalize_groups(1, 2, c, 4, 2, bn, parts, 4, 7, None, st[0], st[1], st[2], st[3], tab, 0))
    # the pool and head forms outside their shapes: W % 8 != 0; a plane that is not a multiple of 4
    s3 = (2, 4, 4, 6)
    z3, a3 = torch.zeros(s3, device=dev), torch.full(s3, B.SENT, device=dev)
    pooled = torch.full((2, 4, 2, 3), B.SENT, device=dev)
    _refused(lambda: ops.bn_train_fwd_pool(z3, a3, pooled, 1, bn, st[0], st[1], st[2], st[3], ws))
    _refused(lambda: ops.bn_relu_bwd_pool(z3, pooled, z3, a3, st[0], st[1], st[2], st[3], vecs[6], vecs[7], vecs[8], ws))
    dl, hw_ = torch.zeros(2, 2, 3, 2, device=dev), torch.zeros(2, c, device=dev)
    _refused(lambda: ops.bn_relu_bwd_head(dl, hw_, z, outs[1], st[0], st[1], st[2], st[3], vecs[6], vecs[7], vecs[8], ws))
    for t in outs + vecs + [a2, a3, pooled, tab]:
        assert bool((t == B.SENT).all())
    assert int(bn.num_batches_tracked.item()) == B.NBT0 and torch.equal(bn.running_mean, op['rm0'].to(dev))
    assert not bool(ws.any())


def test_zz_report_shares():
    print('largest share of its bound per group of checks:', {k: round(v, 3) for k, v in sorted(SHARES.items())})
