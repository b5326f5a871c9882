"""The references of tests/attention_cases.py without a GPU.

1. For every case of every table that tests/test_gpu_attention_paths.py runs, the operator in fp32 aten lies within a QUARTER
   of the bound the GPU test applies to that quantity: the float64 references are the operator, and the bounds leave room
   for a correct fp32 kernel.  Measured here (fp32 aten against float64, of the scale the bound uses):
       1x1 conv        y 3.3e-7, dx (plain, fused, accumulating) 4.4e-7, dw 1.4e-7 (2.7e-7 of the rms scale at R = 1), db 3.3e-7 (rms)
       dilated conv    y 2.3e-7, dx 1.8e-7, dw 1.9e-7, db 3.0e-7 (rms)
       gate            gate / out 1.9e-6 (the offset-mean row; 3.1e-7 at the grid-wrap size, <= 9.4e-8 elsewhere), running
                       statistics 5.0e-8, d t4 2.6e-6, dgamma 2.7e-6 and dbeta 6.6e-6 of the rms scale (both at the
                       grid-wrap size; <= 1.1e-6 elsewhere)
       transposed conv y 2.0e-7, dx 2.0e-7, dw 2.1e-6 (the 4160-pixel row; <= 4.4e-7 elsewhere)
   so every quantity is within 5e-6 (a quarter of 2e-5) resp. 2.5e-5 (a quarter of 1e-4).  Offset-mean gate: kernel
   arithmetic 9.6e-7, naive fp32 one-pass 6.3e-4; grid-wrap gate: kernel arithmetic 1.6e-7, per-thread fp32 sums 3.8e-5.
2. The offset-mean gate case (t4 ~ N(32, 0.5^2), seed fixed in attention_cases.GATE): the kernel's arithmetic (double sums,
   fp32 mean / rstd, fp32 apply) stays within a quarter of the gate bound, a naive fp32 one-pass E[x^2] - mean^2 does not
   stay within the bound.  The grid-wrap gate case does the same against per-thread fp32 partial sums (what float
   accumulators in bn1_stats_kernel would be).
3. Which kernel each row of each table reaches: the dispatch predicates of attention_cases held to expectations written
   out by hand below, and the Layout strides they rest on.  This is the one place where the mapping from case to kernel
   is stated; the GPU test derives its test ids from the same predicates."""
import pytest
import torch
import torch.nn.functional as F

import attention_cases as A
from attention_cases import Layout as L

Q = 0.25


def _ids(c):
    return 'x'.join(str(int(v)) for v in c)


def _check(name, err, bound):
    print('%-28s %.2e (bound %.1e)' % (name, err, bound))
    assert err <= Q * bound, '%s: fp32 aten is %.3e from the float64 reference > a quarter of %.1e' % (name, err, bound)


# ================================================================================================ fp32 aten within a quarter
@pytest.mark.parametrize('case', A.PW + [A.WRAP_PW], ids=_ids)
def test_pw_reference_against_aten_fp32(case):
    n, c, r, h, w = case
    d = A.pw_case(*case)
    xr, wr, br = d['x'].clone().requires_grad_(True), d['w'].view(r, c, 1, 1).clone().requires_grad_(True), \
        d['b'].clone().requires_grad_(True)
    y = F.conv2d(xr, wr, br)
    y.backward(d['dt'])
    _check('y', A.rel_err(y, d['y']), A.CONV_TOL)
    _check('y (no bias)', A.rel_err(F.conv2d(d['x'], d['w'].view(r, c, 1, 1)), d['y_nobias']), A.CONV_TOL)
    _check('dx', A.rel_err(xr.grad, d['dx']), A.CONV_TOL)
    fused = d['gate'][:, None] * d['dout'] + xr.grad
    _check('dx fused', A.rel_err(fused, A.pw_dgrad_ref(d, True, False)), A.CONV_TOL)
    _check('dx fused acc', A.rel_err(d['base'] + fused, A.pw_dgrad_ref(d, True, True)), A.CONV_TOL)
    _check('dx acc', A.rel_err(d['base'] + xr.grad, A.pw_dgrad_ref(d, False, True)), A.CONV_TOL)
    if case == A.WRAP_PW:                  # the weight gradient is not part of the grid-wrap cases
        return
    if r == 1:
        _check('dw (rms)', A.rms_err(wr.grad.view(r, c), d['dw'], A.pw_dw_terms(d)), A.CONV_TOL)
    else:
        _check('dw', A.rel_err(wr.grad.view(r, c), d['dw']), A.CONV_TOL)
    _check('db (rms)', A.rms_err(br.grad, d['db'], A.pw_db_terms(d)), A.CONV_TOL)


@pytest.mark.parametrize('case', A.DCONV + [A.WRAP_DCONV], ids=_ids)
def test_dconv_reference_against_aten_fp32(case):
    dil = case[-1]
    d = A.dconv_case(*case)
    xr, wr, br = (d[k].clone().requires_grad_(True) for k in ('x', 'w', 'b'))
    y = F.conv2d(xr, wr, br, padding=dil, dilation=dil)
    _check('y', A.rel_err(y, d['y']), A.CONV_TOL)
    _check('y (no bias)', A.rel_err(F.conv2d(d['x'], d['w'], None, padding=dil, dilation=dil), d['y_nobias']), A.CONV_TOL)
    if case == A.WRAP_DCONV:               # forward only at the grid-wrap size
        return
    y.backward(d['dy'])
    _check('dx', A.rel_err(xr.grad, d['dx']), A.CONV_TOL)
    _check('dw', A.rel_err(wr.grad, d['dw']), A.CONV_TOL)
    _check('db (rms)', A.rms_err(br.grad, d['db'], A.dconv_db_terms(d)), A.CONV_TOL)


def test_dconv_cases_tell_wrong_filter_indices_apart():
    """Cin != Cout in the first two rows, and the data gradient of a row changes by far more than the bound when the transposed
    form reads the [Cout][Cin][9] filter storage with another index: row-major [Cin][Cout] (the two indices exchanged), or the
    right index order with the wrong row length (co * Cout + ci: invisible at Cin == Cout; modelled on the second row, where
    it stays inside the storage)"""
    assert all(c[1] != c[2] for c in A.DCONV[:2])
    for case in A.DCONV[:2]:
        n, cin, cout, h, w, dil = case
        d = A.dconv_case(*case)
        flat9 = d['w'].double().reshape(cout * cin, 3, 3)
        co, ci = torch.arange(cout)[:, None], torch.arange(cin)[None, :]
        wrong = [flat9[ci * cout + co]]
        if cout < cin:
            assert int((co * cout + ci).max()) < cout * cin
            wrong.append(flat9[co * cout + ci])
        for wt in wrong:
            dx = torch.nn.grad.conv2d_input(d['x'].shape, wt, d['dy'].double(), padding=dil, dilation=dil)
            assert torch.equal(torch.nn.grad.conv2d_input(d['x'].shape, flat9[co * cin + ci], d['dy'].double(), padding=dil, dilation=dil),
                               d['dx'])
            assert A.rel_err(dx, d['dx']) > 1e3 * A.CONV_TOL


@pytest.mark.parametrize('case', A.GATE + [A.WRAP_GATE], ids=_ids)
def test_gate_reference_against_aten_fp32(case):
    d = A.gate_case(*case)
    bn = torch.nn.BatchNorm2d(1, eps=A.EPS, momentum=A.MOMENTUM)
    with torch.no_grad():
        bn.weight.fill_(A.GAMMA); bn.bias.fill_(A.BETA); bn.running_mean.fill_(A.RM0); bn.running_var.fill_(A.RV0)
        bn.num_batches_tracked.fill_(A.NBT0)
    t4 = d['t4'].clone().requires_grad_(True)
    gate = torch.sigmoid(bn(t4))
    out = gate * d['y']
    out.backward(d['dout'])
    _check('gate', A.rel_err(gate[:, 0], d['gate']), A.GATE_TOL)
    _check('out', A.rel_err(out, d['out']), A.GATE_TOL)
    _check('running mean', A.rel_err(bn.running_mean, d['rm']), A.GATE_TOL)
    _check('running var', A.rel_err(bn.running_var, d['rv']), A.GATE_TOL)
    assert int(bn.num_batches_tracked) == d['nbt']
    _check('d t4', A.rel_err(t4.grad, d['dt4']), A.GATE_BWD_TOL)
    _check('dgamma (rms)', A.rms_err(bn.weight.grad, d['dgamma'], d['dgamma_terms']), A.GATE_BWD_TOL)
    _check('dbeta (rms)', A.rms_err(bn.bias.grad, d['dbeta'], d['dbeta_terms']), A.GATE_BWD_TOL)
    with torch.no_grad():
        bn.running_mean.fill_(A.RM0); bn.running_var.fill_(A.RV0)
        bn.eval()
        ge = torch.sigmoid(bn(d['t4']))
    _check('gate (eval)', A.rel_err(ge[:, 0], d['gate_eval']), A.GATE_TOL)
    _check('out (eval)', A.rel_err(ge * d['y'], d['out_eval']), A.GATE_TOL)
    assert float(bn.running_mean) == pytest.approx(A.RM0) and float(bn.running_var) == pytest.approx(A.RV0)


@pytest.mark.parametrize('case', A.CONVT, ids=_ids)
def test_convt_reference_against_aten_fp32(case):
    d = A.convt_case(*case)
    xr, wr = d['x'].clone().requires_grad_(True), d['w'].clone().requires_grad_(True)
    y = F.conv_transpose2d(xr, wr, d['b'], stride=2)
    y.backward(d['dy'])
    _check('y', A.rel_err(y, d['y']), A.CONV_TOL)
    _check('y (no bias)', A.rel_err(F.conv_transpose2d(d['x'], d['w'], None, stride=2), d['y_nobias']), A.CONV_TOL)
    _check('dx', A.rel_err(xr.grad, d['dx']), A.CONV_TOL)
    _check('dw', A.rel_err(wr.grad, d['dw']), A.CONV_TOL)


def test_rms_scale_is_the_scale_of_a_signed_sum():
    t = torch.tensor([[3.0, -4.0], [1.0, 0.0]])
    assert torch.equal(A.rms_scale(t), torch.tensor([5.0, 1.0], dtype=torch.float64))
    assert A.rms_err(torch.tensor([-0.5, 1.0]), torch.tensor([-1.0, 1.0]), t) == pytest.approx(0.1)


# ================================================================================================ the offset-mean gate
def test_offset_mean_gate_discriminates():
    """(a) the kernel's arithmetic stays within a quarter of the gate bound; (b) a naive fp32 one-pass variance does not stay
    within the bound (the seed of the table row was chosen for that)"""
    d = A.gate_case(*A.GATE_OFFSET)
    assert A.GATE_OFFSET[4] and abs(float(d['t4'].mean()) - 32.0) < 0.1
    y = d['y']
    kernel = A.rel_err(A.gate_kernel_arithmetic(d['t4'])[:, None] * y, d['out'])
    naive = A.rel_err(A.gate_naive_fp32(d['t4'])[:, None] * y, d['out'])
    print('offset-mean gate: kernel arithmetic %.2e, naive fp32 one-pass %.2e (bound %.1e)' % (kernel, naive, A.GATE_TOL))
    assert kernel <= Q * A.GATE_TOL
    assert naive > A.GATE_TOL


def test_wrap_gate_discriminates_per_thread_fp32_sums():
    """at the grid-wrap size every thread of the 1024-thread statistics block sums 5120 elements: with double sums the gate is
    within a quarter of the bound, with one fp32 pair of running sums per thread it is outside the bound"""
    d = A.gate_case(*A.WRAP_GATE)
    y = d['y']
    kernel = A.rel_err(A.gate_kernel_arithmetic(d['t4'])[:, None] * y, d['out'])
    lanes = A.rel_err(A.gate_naive_fp32(d['t4'], lanes=1024)[:, None] * y, d['out'])
    print('grid-wrap gate: kernel arithmetic %.2e, per-thread fp32 sums %.2e (bound %.1e)' % (kernel, lanes, A.GATE_TOL))
    assert kernel <= Q * A.GATE_TOL
    assert lanes > A.GATE_TOL


# ================================================================================================ case -> kernel
ORDER = ('dense', 'slice', 'pad4', 'pad1', 'pad2')
# V: the <4> (16-byte) instantiation, S: the <1> instantiation, per layout kind in ORDER
PW_EXPECT = {(2, 32, 2, 4, 6): 'VVVSS',      # HW = 24
             (2, 20, 3, 3, 5): 'SSSSS',      # HW = 15
             (2, 300, 1, 2, 2): 'VVVSS',     # HW = 4
             (2, 4, 300, 2, 2): 'VVVSS',
             (5, 2, 2, 1024, 1024): 'VVVSS'}
GATE_EXPECT = {(2, 8, 12, 10): 'VVVSS',      # HW = 120
               (2, 5, 3, 5): 'SSSSS',        # HW = 15
               (3, 4, 20, 20): 'VVVSS',      # HW = 400
               (2, 3, 2, 4): 'VVVSS',        # HW = 8
               (5, 2, 1024, 1024): 'VVVSS'}


def _vs(name):
    return {'<4>': 'V', '<1>': 'S'}[name[-3:]]


@pytest.mark.parametrize('case', A.PW + [A.WRAP_PW], ids=_ids)
def test_pw_dispatch_table(case):
    n, c, r, h, w = case
    for kind, exp in zip(ORDER, PW_EXPECT[case]):
        rd, wr = A.KINDS[kind]
        xs, ys = (n, c, h, w), (n, r, h, w)
        assert _vs(A.pw_fwd_kernel(h * w, A.bs_of(rd, xs), A.bs_of(wr, ys))) == exp, ('fwd', kind)
        assert _vs(A.pw_dgrad_kernel(h * w, A.bs_of(rd, ys), A.bs_of(wr, xs))) == exp, ('dgrad', kind)
        assert _vs(A.pw_dgrad_kernel(h * w, A.bs_of(rd, ys), A.bs_of(wr, xs), A.bs_of(rd, xs))) == exp, ('fused dgrad', kind)


def test_one_operand_on_pad2_takes_the_scalar_kernel():
    """each stride of each predicate on its own: the others dense, HW % 4 == 0"""
    n, c, r, h, w = A.PW_PAD2
    xs, ys, hw = (n, c, h, w), (n, r, h, w), h * w
    dx_, dy_ = A.bs_of('dense', xs), A.bs_of('dense', ys)
    px, py = A.bs_of('pad2', xs), A.bs_of('pad2', ys)
    assert (dx_ % 4, dy_ % 4, px % 4, py % 4, hw % 4) == (0, 0, 2, 2, 0)
    assert A.pw_fwd_kernel(hw, dx_, dy_) == 'pw_fwd_kernel<4>'
    assert A.pw_fwd_kernel(hw, px, dy_) == A.pw_fwd_kernel(hw, dx_, py) == 'pw_fwd_kernel<1>'
    assert A.pw_dgrad_kernel(hw, dy_, dx_) == A.pw_dgrad_kernel(hw, dy_, dx_, dx_) == 'pw_dgrad_kernel<4>'
    assert A.pw_dgrad_kernel(hw, py, dx_) == A.pw_dgrad_kernel(hw, dy_, px) == 'pw_dgrad_kernel<1>'
    assert A.pw_dgrad_kernel(hw, dy_, dx_, px) == 'pw_dgrad_kernel<1>'            # dout counts only when it is passed
    assert A.sa_mul_kernel(hw, dx_, dx_) == 'sa_mul_kernel<4>'
    assert A.sa_mul_kernel(hw, px, dx_) == A.sa_mul_kernel(hw, dx_, px) == 'sa_mul_kernel<1>'
    assert A.sa_mul_bwd_kernel(hw, dx_, dx_) == 'sa_mul_bwd_kernel<4>'
    assert A.sa_mul_bwd_kernel(hw, px, dx_) == A.sa_mul_bwd_kernel(hw, dx_, px) == 'sa_mul_bwd_kernel<1>'


@pytest.mark.parametrize('case', A.GATE + [A.WRAP_GATE], ids=_ids)
def test_gate_dispatch_table(case):
    n, c, h, w = case[:4]
    s = (n, c, h, w)
    for kind, exp in zip(ORDER, GATE_EXPECT[s]):
        rd, wr = A.KINDS[kind]
        assert _vs(A.sa_mul_kernel(h * w, A.bs_of(rd, s), A.bs_of(wr, s))) == exp, ('sa_mul', kind)
        assert _vs(A.sa_mul_bwd_kernel(h * w, A.bs_of(rd, s), A.bs_of(rd, s))) == exp, ('sa_gate_bwd', kind)


def test_loops_and_wraps_the_tables_reach():
    """staging loops (256 threads), the 1024-thread reductions, the 4096 x 256 grid cap"""
    assert A.PW[2][1] > 256 and A.PW[2][2] == 1             # forward stages C filter values; R = 1 is the conv4 form
    assert A.PW[3][2] > 256                                  # dgrad stages R
    assert A.DCONV[3][1] * 9 > 256 and A.DCONV[3][2] * 9 > 256      # forward stages Cin * 9, the transposed form Cout * 9
    n, cin, cout, h, w, dil = A.DCONV[1]
    assert dil >= h and dil >= w                             # only the centre tap is inside the plane
    assert [c[0] * c[2] * c[3] for c in A.GATE] == [240, 30, 1200, 16]          # M against the 1024 threads
    n, c, r, h, w = A.WRAP_PW
    assert n * h * w // 4 > A.GRID_CAP and -(-n * h * w // A.GRID_CAP) == 5     # vector kernels: 2 trips, scalar: 5
    assert A.WRAP_DCONV[:5] == A.WRAP_PW and A.WRAP_GATE[:1] + A.WRAP_GATE[2:4] == (n, h, w)


# (splits, pixels per split, non-empty splits) of the transposed conv's weight gradient
CONVT_EXPECT = {(2, 24, 40, 10, 10): (13, 16, 13),     # K chunk 96 .. 111 straddles the image boundary at 100; last chunk 8 wide
                (1, 3, 3, 1, 1): (1, 16, 1),
                (1, 70, 5, 3, 7): (2, 16, 2),          # 1024 / 2 tiles = 512, capped by kmax = ceil(21 / 16) = 2
                (2, 17, 33, 5, 13): (9, 16, 9),        # 1024 / 3 tiles = 342, capped by kmax = ceil(130 / 16) = 9; last split 2 wide
                (1, 8, 4, 64, 65): (256, 32, 130)}     # ceil(4160 / 256) = 17 -> 32 per split: 126 empty splits


@pytest.mark.parametrize('case', A.CONVT, ids=_ids)
def test_convt_split_table(case):
    assert A.convt_splits(*case) == CONVT_EXPECT[case]
    n, ci, co, h, w = case
    s, per, live = CONVT_EXPECT[case]
    assert (live - 1) * per < n * h * w <= live * per and live <= s


def test_convt_tile_shapes():
    n, ci, co, h, w = A.CONVT[1]
    assert 4 * co < 16 and ci < 16 and h * w < 64                       # dgrad K = 12 < TK, every tile dimension partial
    assert A.CONVT[2][1] > 64 and A.CONVT[2][1] % 16 != 0                # two M tiles, ragged K in the forward
    assert 128 < 4 * A.CONVT[3][2] <= 192                                # three N tiles in wgrad


@pytest.mark.parametrize('kind', sorted(A.KINDS))
def test_layout_strides_of_the_kinds(kind):
    """batch strides mod 4 of the kinds on a C H W % 4 == 0 shape, and N == 1 hiding the padding"""
    rd, wr = A.KINDS[kind]
    shape = (2, 3, 4, 6)
    exp = {'dense': (0, 0), 'slice': (0, 0), 'pad4': (0, 0), 'pad1': (1, 1), 'pad2': (2, 2)}[kind]
    assert (A.bs_of(rd, shape) % 4, A.bs_of(wr, shape) % 4) == exp
    assert A.bs_of(rd, (1, 3, 4, 6)) == 72
    lr, lw = L(rd, shape), L(wr, shape)
    if kind == 'slice':
        assert (lr.kind, lw.kind, lr.bs, lw.bs, lr.offset - lw.offset) == ('hi', 'lo', 144, 144, 72)
    flat, v = lw.put(torch.randn(shape), 'cpu')
    assert lw.intact(flat) and v.stride(0) == lw.bs
