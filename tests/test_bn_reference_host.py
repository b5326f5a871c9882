"""Makes tests/bn_cases.py binding, without a GPU: the path predictor reaches every kernel instantiation the tables name and every
row reaches the path it is annotated with; reference 2 (the kernel's contract in float64) under exact coefficients reproduces
reference 1 (the float64 operator and its autograd), also without the ReLU and through a negative and a zero gamma; the mask claim
of reference 2 holds in rational arithmetic; a plain fp32 evaluation of the kernels' arithmetic (bn_cases.emulate: one arithmetic
for every form, no kernel keeps an fp32 partial sum) stays inside every bound; and no elementwise bound is vacuous.

Largest share of its bound the fp32 emulation uses, over all rows (test_fp32_emulation_inside_bounds prints them with -s):
    coefficients and running statistics vs reference 1      0.97
    a vs reference 2                                        1.00
    dz elementwise vs reference 2                           0.91
    dgamma / dbeta                                          0.98
    dbias                                                   0.16
The bounds carry no slack beyond the roundings they count, and among the 10^5 .. 10^7 elements of a row some element uses nearly the
whole half spacing of each rounding at once: a share close to 1 is the sign of a count without a spare rounding, not of a missing
one (that would show as a share above 1).  The `one half` rule
of thumb holds for the one bound whose terms cannot all be extreme together, dbias.  The emulation rounds where the kernel rounds;
aten's own fp32 BatchNorm accumulates in fp32 and evaluates (z - mean) * invstd * w + b, another arithmetic than the one the
bounds count -- it is not held to them."""
import fractions

import pytest
import torch

import bn_cases as B

SHARES = {}


def _note(group, value):
    SHARES[group] = max(SHARES.get(group, 0.0), value)


def test_tables_reach_every_instantiation():
    reached = set()
    for row in B.ROWS:
        fwd, bwd, _ = B.row_plans(row)
        assert B.path_of(fwd) == row.fwd and B.path_of(bwd) == row.bwd, row.name
        reached |= {(p.form, p.V, p.Q) for p in (fwd, bwd)}
        for kind in row.kinds:
            assert kind in B.kinds_for(row.shape), (row.name, kind)
    missing = [x for x in B.NEEDED if x not in reached]
    assert not missing, missing
    for name, m, groups, c, h, w, kinds, path in B.GROUP_ROWS:
        bz, ba = (B.batch_stride(k, (m * groups, c, h, w)) for k in kinds)
        assert B.path_of(B.predict_fwd((m, c, h, w), bz, ba, groups=groups)) == path, name
    widths = set()
    for shape, kinds in B.layout_sweep():
        row = B.Row('sweep', shape, kinds, None, None, B.F4, False)
        fwd, bwd, ap = B.row_plans(row)
        assert fwd.form != 'error' and bwd.form != 'error'
        widths |= {(fwd.form, fwd.V), (bwd.form, bwd.V), ('apply', ap)}
    assert {('one-pass', 8), ('one-pass', 4), ('two-pass', 1), ('apply', 4), ('apply', 1)} <= widths
    # one tensor's stride alone decides: z dense, only dz on pad4 -> the forward stays 8 wide, the backward goes to 4
    fwd, bwd, _ = B.row_plans(B.Row('x', (2, 6, 32, 40), ('dense', 'dense', 'dense', 'pad4'), None, None, B.F4, False))
    assert (fwd.V, bwd.V) == (8, 4)


def test_predictor_states_the_plans_of_the_tables():
    """figures the case tables quote, from the predictor"""
    p = B.row_plans(B.ROW['v4_by_stride'])[0]
    assert (p.S, p.per, 640 - (p.S - 1) * p.per) == (3, 214, 212)
    assert B.row_plans(B.ROW['v4_s1'])[0].per == 12
    p = B.row_plans(B.ROW['v8_q2'])[0]
    assert (p.per, p.Q) == (378, 2)
    p = B.row_plans(B.ROW['tp_v1_plane'])[0]
    assert p.splits * p.per > 3 * 37 * 41 > (p.splits - 1) * p.per          # a ragged last split, none empty
    assert 17 * 512 * 512 // 8 == 557056 > 256 * 256 * 8
    assert 4 * 640 * 64 * 64 > 9 << 20
    # the narrow limit is the only thing that separates the bf16 call of that shape from the fp32 call
    assert B.predict_fwd((4, 640, 64, 64), 640 * 4096, 640 * 4096).form == 'one-pass'
    assert B.predict_fwd((8, 2, 15, 15), 450, 450, groups=13).splits == 96 // 13 < B.pick_splits(8, 2, 225)
    assert B.predict_fwd((8, 2, 15, 15), 450, 450, groups=97).form == 'error'
    assert B.epoch_step(B.row_plans(B.ROW['v4_s2'])[0], 3) == 3 and B.epoch_step(B.row_plans(B.ROW['v4_s1'])[0]) == 0
    assert B.epoch_step(B.row_plans(B.ROW['tp_v4'])[0]) == 0


HOST_ROWS = B.SMALL + ['v8_q2', 'tp_v4', 'tp_v8']          # every form and width; the other big rows differ in Q and S only


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('name', HOST_ROWS)
def test_contract_reproduces_operator(name, relu):
    """reference 2 under the exact (float64) coefficients == reference 1.  The one difference is stated in the contract: c0 and c1
    are fp32 values, so dz may differ by |scale| (u |c0| + |xhat| u |c1|); everything else agrees to float64 rounding."""
    row = B.ROW[name]
    op = B.row_operands(row)
    r1 = B.ref_operator(op['z'], op['gamma'], op['beta'], op['rm0'], op['rv0'], op['dA'], relu)
    if r1['n'] == 1:
        assert torch.equal(r1['var'], torch.zeros_like(r1['var']))
        assert torch.allclose(r1['rv'], (1 - B.MOM) * op['rv0'].double(), rtol=0, atol=0)
        return
    r2 = B.ref_contract(op['z'], op['dA'], r1['mean'], r1['rstd'], r1['scale'], r1['shift'], relu)
    if relu:
        assert B._clear_of_zero(op['z'], r2['y'], B._v(r1['scale']), B._v(r1['shift'])).all()
        assert torch.equal(r2['mask'], r1['a'] > 0)
    tiny = 1e-11
    assert B.share(r2['a'], r1['a'], tiny * (r1['a'].abs() + 1)) <= 1
    sc = B._v(r1['scale'].abs())
    lim = sc * B.U * (B._v(r2['c0'].abs()) + r2['xhat'].abs() * B._v(r2['c1'].abs())) + tiny * (r1['dz'].abs() + 1)
    assert B.share(r2['dz'], r1['dz'], lim) <= 1
    n = r1['n']
    assert B.share(r2['dgamma'], r1['dgamma'], tiny * n) <= 1 and B.share(r2['dbeta'], r1['dbeta'], tiny * n) <= 1
    c = op['z'].shape[1]
    if c >= 3:                                   # the negative and the zero gamma were part of that
        assert op['gamma'][1] < 0 and op['gamma'][2] == 0 and r2['dz'][:, 2].abs().max() == 0


def _frac(x):
    return fractions.Fraction(float(x))


@pytest.mark.parametrize('name', B.SMALL)
def test_mask_claim_exact(name):
    """for the elements closest to zero of every small row, under the fp32 coefficients of the emulation: the sign of the float64
    z * scale + shift is the sign of the exact rational value, and that value is either 0 or far above the smallest normal
    fp32 number -- so the fp32 fmaf (one rounding of the exact value) has the same sign: the two masks are one"""
    row = B.ROW[name]
    op = B.row_operands(row)
    fwd, bwd, _ = B.row_plans(row)
    em = B.emulate(op['z'], op['dA'], op['gamma'], op['beta'], op['rm0'], op['rv0'])
    z = op['z']
    y = z.double() * B._v(em['scale']) + B._v(em['shift'])
    order = y.abs().flatten().argsort()[:48]
    cidx = (order // (z.shape[2] * z.shape[3])) % z.shape[1]
    for i, c in zip(order.tolist(), cidx.tolist()):
        exact = _frac(z.flatten()[i]) * _frac(em['scale'][c]) + _frac(em['shift'][c])
        y64 = float(y.flatten()[i])
        assert (exact > 0) == (y64 > 0) and (exact < 0) == (y64 < 0)
        assert exact == 0 or abs(exact) > fractions.Fraction(2) ** -100
        prod = _frac(z.flatten()[i]) * _frac(em['scale'][c])
        assert fractions.Fraction(float(z.flatten()[i]) * float(em['scale'][c])) == prod        # the product is exact in float64
        assert (torch.tensor(float(exact), dtype=torch.float64).float().item() > 0) == (exact > 0)


def _check_emulation(op, fwd, bwd, relu, what):
    r1 = B.ref_operator(op['z'], op['gamma'], op['beta'], op['rm0'], op['rv0'], relu=relu)
    em = B.emulate(op['z'], op['dA'], op['gamma'], op['beta'], op['rm0'], op['rv0'], relu)
    sb = B.stat_bounds(r1, op['gamma'], op['beta'], op['rm0'], op['rv0'])
    for k in sb:
        s = B.share(em[k], r1[k], sb[k])
        _note('coefficients', s)
        assert s <= 1, (what, k, s)
    r2 = B.ref_contract(op['z'], op['dA'], em['mean'], em['rstd'], em['scale'], em['shift'], relu)
    assert torch.equal(r2['mask'], em['a'] > 0) or not relu
    s = B.share(em['a'], r2['a'], B.a_bound(op['z'], r2['y'], em['scale'], em['shift']))
    _note('a', s)
    assert s <= 1, (what, 'a', s)
    bb = B.bwd_bounds(r2, em['scale'])
    for k in ('dz', 'dgamma', 'dbeta', 'dbias'):
        s = B.share(em[k], r2[k], bb[k])
        _note('dz' if k == 'dz' else 'dbias' if k == 'dbias' else 'sums', s)
        assert s <= 1, (what, k, s)


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('name', HOST_ROWS)
def test_fp32_emulation_inside_bounds(name, relu):
    row = B.ROW[name]
    fwd, bwd, _ = B.row_plans(row)
    _check_emulation(B.row_operands(row), fwd, bwd, relu, name)
    print('shares so far:', {k: round(v, 3) for k, v in SHARES.items()})


@pytest.mark.parametrize('shape,tag,what', B.STRESS)
def test_fp32_emulation_inside_bounds_stress(shape, tag, what):
    op = B.stress_operands(shape, what)
    bs = shape[1] * shape[2] * shape[3]
    _check_emulation(op, B.predict_fwd(shape, bs, bs), B.predict_bwd(shape, bs, bs, bs), True, what)


@pytest.mark.parametrize('name', [n for n in HOST_ROWS if B.ROW[n].shape != (1, 3, 1, 1)])
def test_bounds_not_vacuous(name):
    """a reference with one unit of V values of channel 0 zeroed, and one that takes c0 from the neighbouring channel, leave the
    elementwise bounds (a unit is zeroed where the reference holds a non-zero value)"""
    row = B.ROW[name]
    op = B.row_operands(row)
    fwd, bwd, _ = B.row_plans(row)
    em = B.emulate(op['z'], op['dA'], op['gamma'], op['beta'], op['rm0'], op['rv0'])
    r2 = B.ref_contract(op['z'], op['dA'], em['mean'], em['rstd'], em['scale'], em['shift'])
    ab = B.a_bound(op['z'], r2['y'], em['scale'], em['shift'])
    bb = B.bwd_bounds(r2, em['scale'])
    n, c, h, w = row.shape
    for key, ref, bound, v in (('a', r2['a'], ab, fwd.V), ('dz', r2['dz'], bb['dz'], bwd.V)):
        plane = ref[:, 0].reshape(n, -1)
        units = plane.reshape(n, -1, v)
        hit = (units != 0).any(2).nonzero()[0]
        mut = units.clone()
        mut[hit[0], hit[1]] = 0.0
        assert B.share(mut.reshape(n, -1), plane, bound[:, 0].reshape(n, -1)) > 1, key
    if c >= 2:
        other = torch.roll(r2['c0'], 1)
        assert (other != r2['c0']).any()
        mut = B._v(em['scale']) * (r2['dy'] - B._v(other) - r2['xhat'] * B._v(r2['c1']))
        live = [k for k in range(c) if em['scale'][k] != 0 and other[k] != r2['c0'][k]]
        for k in live:
            assert B.share(mut[:, k], r2['dz'][:, k], bb['dz'][:, k]) > 1, k


def test_parts_reference_and_eval_fold():
    """the synthesised conv-epilogue statistics: the float64 sum of the fp32 parts gives the true statistics of z to within the
    bound the parts' own rounding implies (one rounding per entry), for every part count, with and without a conv bias"""
    shape = (5, 8, 20, 20)
    op = B.operands(shape)
    n = 5 * 400
    cb = torch.linspace(-1.0, 1.0, 8)
    for nparts in B.PARTS_N:
        for bias in (cb, None):
            parts = B.make_parts(op['z'], bias, nparts, stride=nparts + 3)
            assert torch.isnan(parts[:, nparts:]).all() and not torch.isnan(parts[:, :nparts]).any()
            rp = B.ref_from_parts(parts, 0, nparts, n, bias, op['gamma'], op['beta'])
            r1 = B.ref_operator(op['z'], op['gamma'], op['beta'])
            dm = B.U * rp['P1']
            dvar = B.U * rp['A2'] + 2 * rp['mean_pre'].abs() * dm
            assert ((rp['mean'] - r1['mean']).abs() <= dm + 1e-15).all()
            assert ((rp['var'] - r1['var']).abs() <= dvar + 1e-15).all()
    (sc, sh, fb), (bs, bsh, bf) = B.eval_fold_ref(op['gamma'], op['beta'], op['rm0'], op['rv0'], cb)
    rstd = 1.0 / torch.sqrt((op['rv0'] + torch.tensor(B.EPS)))
    sc32 = op['gamma'] * rstd
    sh32 = op['beta'] - op['rm0'] * sc32
    assert B.share(sc32, sc, bs) <= 1 and B.share(sh32, sh, bsh) <= 1 and B.share(cb * sc32 + sh32, fb, bf + B.U * fb.abs()) <= 1
