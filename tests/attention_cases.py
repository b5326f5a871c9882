"""References, dispatch predicates and inputs of tests/test_gpu_attention_paths.py (the Spatial_Attention branch of
aide_amd/csrc/attention.hip and the ConvTranspose2d(2, 2) kernels of aide_amd/csrc/convt.hip), validated without a GPU by
tests/test_attention_reference_host.py.  Everything here is plain torch on the CPU:

  * 1x1 conv: float64 F.conv2d and its autograd, plus the fused data gradient base * acc + gate[:, None] * dout + W^T dt;
  * dilated 3x3 conv: float64 F.conv2d(padding=d, dilation=d) with Cin != Cout and its autograd;
  * gate: sigmoid(F.batch_norm(t4)) * y in float64, training (running mean, unbiased running variance, counter, d t4,
    dgamma, dbeta) and eval mode;
  * transposed conv: float64 F.conv_transpose2d(stride=2) and its autograd.

Every case takes fp32-valued inputs, casts them to float64 and is computed once (lru_cache on the case tuple).  Results
that are ONE sum of randomly signed terms (dgamma, dbeta, a bias gradient, the weight gradient of the R = 1 conv) are
compared on the scale sqrt(sum t_i^2) of their float64 terms (rms_err): |ref| itself is arbitrarily small for an unlucky
seed.  Everything else is compared on max |ref| (spatial_cases.rel_err).

Layouts, sentinels and the error measure are spatial_cases'."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from spatial_cases import Layout, SENT, GUARD, rel_err, assert_close  # noqa: F401  (re-exported to the two test files)

CONV_TOL = 2e-5            # 1x1, dilated and transposed conv outputs and gradients (_close of test_gpu_attention.py / test_gpu_kernels.py)
GATE_TOL = 2e-5            # gate output and running statistics
GATE_BWD_TOL = 1e-4        # d t4, dgamma, dbeta

# layout kind of a test -> (layout of the operands the kernel reads, layout of the operands it writes)
KINDS = {'dense': ('dense', 'dense'), 'slice': ('hi', 'lo'), 'pad4': ('pad4', 'pad4'), 'pad1': ('pad1', 'pad1'),
         'pad2': ('pad2', 'pad2')}


# ------------------------------------------------------------------------------------------------ error measures
def rms_scale(terms):
    """sqrt(sum_k terms[..., k]^2): the magnitude a sum of randomly signed terms has"""
    return terms.double().pow(2).sum(-1).sqrt()


def rms_err(got, ref, terms):
    """max_i |got_i - ref_i| / sqrt(sum_k terms[i, k]^2) in float64; terms: ref.shape + (K,)"""
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    scale = rms_scale(terms).reshape(-1)
    assert scale.shape == ref.shape
    return ((got - ref).abs() / (scale + 1e-30)).max().item()


def assert_close_rms(got, ref, terms, rtol, what=''):
    err = rms_err(got, ref, terms)
    assert err <= rtol, '%s: max abs err %.3e of the rms scale of its terms > %.3e' % (what, err, rtol)


# ------------------------------------------------------------------------------------------------ dispatch predicates
def eff_bs(lay):
    """the batch stride the entry sees: ops.planes replaces it by C*H*W when N == 1"""
    n, c, h, w = lay.shape
    return c * h * w if n == 1 else lay.bs


def pw_fwd_kernel(hw, x_bs, y_bs):
    """aide_pwconv_fwd"""
    return 'pw_fwd_kernel<4>' if hw % 4 == 0 and x_bs % 4 == 0 and y_bs % 4 == 0 else 'pw_fwd_kernel<1>'


def pw_dgrad_kernel(hw, dt_bs, dx_bs, dout_bs=None):
    """aide_pwconv_dgrad; dout_bs None: the plain form (no gate / dout)"""
    vec = hw % 4 == 0 and dt_bs % 4 == 0 and dx_bs % 4 == 0 and (dout_bs is None or dout_bs % 4 == 0)
    return 'pw_dgrad_kernel<4>' if vec else 'pw_dgrad_kernel<1>'


def sa_mul_kernel(hw, y_bs, out_bs):
    """aide_sa_mul"""
    return 'sa_mul_kernel<4>' if hw % 4 == 0 and y_bs % 4 == 0 and out_bs % 4 == 0 else 'sa_mul_kernel<1>'


def sa_mul_bwd_kernel(hw, dout_bs, y_bs):
    """aide_sa_gate_bwd (its first kernel; bn1_bwd_reduce_kernel and bn1_bwd_apply_kernel always follow)"""
    return 'sa_mul_bwd_kernel<4>' if hw % 4 == 0 and dout_bs % 4 == 0 and y_bs % 4 == 0 else 'sa_mul_bwd_kernel<1>'


def convt_splits(n, ci, co, h, w):
    """wgrad_splits of convt.hip -> (splits, pixels per split, non-empty splits)"""
    tiles = ((ci + 63) // 64) * ((co * 4 + 63) // 64)
    s = (1024 + tiles - 1) // tiles
    k = n * h * w
    s = max(1, min(s, (k + 15) // 16, 256))
    per = ((k + s - 1) // s + 15) // 16 * 16
    return s, per, (k + per - 1) // per


def bs_of(kind, shape):
    return eff_bs(Layout(kind, shape))


# ------------------------------------------------------------------------------------------------ tables
# 1x1 conv (n, c, r, h, w)
PW = [(2, 32, 2, 4, 6),        # HW = 24: vector on dense / slice / pad4, scalar on pad1 / pad2
      (2, 20, 3, 3, 5),        # HW = 15: scalar on every layout
      (2, 300, 1, 2, 2),       # C = 300 > 256: second trip of the forward's filter-staging loop; R = 1, the conv4 form
      (2, 4, 300, 2, 2)]       # R = 300 > 256: second trip of the dgrad's staging loop
PW_PAD2 = (2, 32, 2, 4, 6)     # the shape of the "one operand alone on pad2" cases
# dilated conv (n, cin, cout, h, w, dil)
DCONV = [(2, 3, 5, 6, 7, 4),   # Cin != Cout
         (1, 5, 3, 4, 4, 4),   # Cin != Cout; dilation >= plane: only the centre tap is live
         (2, 2, 2, 12, 9, 1),  # dilation 1
         (1, 32, 32, 4, 4, 4),  # Cin * 9 = 288 > 256: second trip of the staging loop
         (2, 4, 4, 5, 16, 2)]
# gate (n, c, h, w, offset, seed); offset: t4 ~ N(32, 0.5^2) instead of N(0.3, 1.5^2)
GATE = [(2, 8, 12, 10, False, 0),    # HW = 120: vector
        (2, 5, 3, 5, False, 0),      # HW = 15: sa_mul_kernel<1>, sa_mul_bwd_kernel<1>
        (3, 4, 20, 20, True, 2),     # M = 1200 > 1024: second trip of the 1024-thread reductions, offset-mean input
        (2, 3, 2, 4, False, 0)]      # M = 16 < 1024
GATE_OFFSET = GATE[2]
# more than 4096 x 256 work items on the vector kernels (N H W / 4 = 1 310 720), five trips on the scalar ones
WRAP_PW = (5, 2, 2, 1024, 1024)
WRAP_DCONV = (5, 2, 2, 1024, 1024, 4)
WRAP_GATE = (5, 2, 1024, 1024, True, 1)
GRID_CAP = 4096 * 256
# transposed conv (n, ci, co, h, w)
CONVT = [(2, 24, 40, 10, 10),  # image boundary inside a K chunk of wgrad, ragged M / N tiles
         (1, 3, 3, 1, 1),      # every tile dimension partial; dgrad K = 12 < 16
         (1, 70, 5, 3, 7),     # two M tiles in dgrad / wgrad, the second partial; Ci % 16 != 0
         (2, 17, 33, 5, 13),   # 4 Co = 132: three N tiles in wgrad; N H W = 130: split count capped by kmax = 9
         (1, 8, 4, 64, 65)]    # N H W = 4160: 256 splits of 32 pixels, 126 of them empty
CONVT_KINDS = {'dense': ('dense', 'dense'), 'slice': ('hi', 'lo'), 'xpad4': ('pad4', 'dense'), 'xpad1': ('pad1', 'dense'),
               'xpad1-lo': ('pad1', 'lo')}        # (x and dx, y and dy)


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 3) * 7919 ** (i % 3) * int(k) for i, k in enumerate(key)) % (2 ** 31)))


# ------------------------------------------------------------------------------------------------ 1x1 conv
@functools.lru_cache(maxsize=None)
def pw_case(n, c, r, h, w):
    """-> dict: fp32 x [n,c,h,w], w [r,c], b [r], dt [n,r,h,w], gate [n,h,w], dout, base [n,c,h,w] and float64
    y, y_nobias, dx (= W^T dt), dw [r,c], db [r]"""
    g = _gen(1, n, c, r, h, w)
    d = dict(x=torch.randn(n, c, h, w, generator=g), w=torch.randn(r, c, generator=g) * (1.0 / c ** 0.5),
             b=torch.randn(r, generator=g), dt=torch.randn(n, r, h, w, generator=g), gate=torch.rand(n, h, w, generator=g),
             dout=torch.randn(n, c, h, w, generator=g), base=torch.randn(n, c, h, w, generator=g))
    xr = d['x'].double().requires_grad_(True)
    wr = d['w'].double().view(r, c, 1, 1).clone().requires_grad_(True)
    br = d['b'].double().clone().requires_grad_(True)
    y = F.conv2d(xr, wr, br)
    y.backward(d['dt'].double())
    d['y'], d['dx'], d['dw'], d['db'] = y.detach(), xr.grad, wr.grad.view(r, c), br.grad
    d['y_nobias'] = d['y'] - d['b'].double().view(1, r, 1, 1)
    return d


def pw_dgrad_ref(d, fused, acc):
    """float64 base * acc + gate[:, None] * dout * fused + W^T dt"""
    ref = d['dx']
    if fused:
        ref = ref + d['gate'].double()[:, None] * d['dout'].double()
    if acc:
        ref = ref + d['base'].double()
    return ref


def pw_db_terms(d):
    """[r, n*hw]: db[r] = sum_{n,p} dt[n][r][p]"""
    r = d['dt'].shape[1]
    return d['dt'].double().transpose(0, 1).reshape(r, -1)


def pw_dw_terms(d):
    """[r, c, n*hw]: dw[r][c] = sum_{n,p} dt[n][r][p] x[n][c][p]"""
    n, c = d['x'].shape[:2]
    r = d['dt'].shape[1]
    t = d['dt'].double().reshape(n, r, 1, -1) * d['x'].double().reshape(n, 1, c, -1)
    return t.permute(1, 2, 0, 3).reshape(r, c, -1)


# ------------------------------------------------------------------------------------------------ dilated conv
@functools.lru_cache(maxsize=None)
def dconv_case(n, cin, cout, h, w, dil):
    """-> dict: fp32 x [n,cin,h,w], w [cout,cin,3,3], b [cout], dy [n,cout,h,w] and float64 y, y_nobias, dx, dw, db"""
    g = _gen(2, n, cin, cout, h, w, dil)
    d = dict(x=torch.randn(n, cin, h, w, generator=g), w=torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (3.0 * cin ** 0.5)),
             b=torch.randn(cout, generator=g), dy=torch.randn(n, cout, h, w, generator=g))
    xr, wr, br = (d[k].double().clone().requires_grad_(True) for k in ('x', 'w', 'b'))
    y = F.conv2d(xr, wr, br, padding=dil, dilation=dil)
    y.backward(d['dy'].double())
    d['y'], d['dx'], d['dw'], d['db'] = y.detach(), xr.grad, wr.grad, br.grad
    d['y_nobias'] = d['y'] - d['b'].double().view(1, cout, 1, 1)
    return d


def dconv_db_terms(d):
    """[cout, n*hw]"""
    cout = d['dy'].shape[1]
    return d['dy'].double().transpose(0, 1).reshape(cout, -1)


# ------------------------------------------------------------------------------------------------ gate
GAMMA, BETA, RM0, RV0, NBT0, EPS, MOMENTUM = 1.3, -0.2, 0.1, 0.7, 3, 1e-5, 0.1


def gate_inputs(n, c, h, w, offset, seed):
    g = _gen(3, n, c, h, w, int(offset), seed)
    t4 = torch.randn(n, 1, h, w, generator=g)
    t4 = t4 * 0.5 + 32.0 if offset else t4 * 1.5 + 0.3
    return t4, torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)


@functools.lru_cache(maxsize=None)
def gate_case(n, c, h, w, offset=False, seed=0):
    """-> dict: fp32 t4 [n,1,h,w], y, dout [n,c,h,w]; float64, training mode: gate [n,h,w], out, rm, rv (after one step from
    RM0 / RV0), nbt, dt4, dgamma, dbeta and the terms of the two sums (dgamma_terms, dbeta_terms: [1, M]); eval mode (running
    statistics RM0 / RV0): gate_eval, out_eval"""
    t4, y, dout = gate_inputs(n, c, h, w, offset, seed)
    d = dict(t4=t4, y=y, dout=dout)
    t = t4.double().requires_grad_(True)
    gam, bet = torch.tensor([GAMMA], dtype=torch.float64, requires_grad=True), torch.tensor([BETA], dtype=torch.float64, requires_grad=True)
    rm, rv = torch.tensor([RM0], dtype=torch.float64), torch.tensor([RV0], dtype=torch.float64)
    z = F.batch_norm(t, rm, rv, gam, bet, True, MOMENTUM, EPS)
    gate = torch.sigmoid(z)
    out = gate * y.double()
    out.backward(dout.double())
    d.update(gate=gate.detach()[:, 0], out=out.detach(), rm=rm, rv=rv, nbt=NBT0 + 1, dt4=t.grad, dgamma=gam.grad, dbeta=bet.grad)
    a = t4.double()
    mean, var = a.mean(), a.var(unbiased=False)
    xhat = ((a - mean) / torch.sqrt(var + EPS))[:, 0]
    gd = d['gate']
    ds = (dout.double() * y.double()).sum(1) * gd * (1.0 - gd)
    d['dbeta_terms'], d['dgamma_terms'] = ds.reshape(1, -1), (ds * xhat).reshape(1, -1)
    with torch.no_grad():
        ze = F.batch_norm(a, torch.tensor([RM0], dtype=torch.float64), torch.tensor([RV0], dtype=torch.float64),
                          gam, bet, False, MOMENTUM, EPS)
        d['gate_eval'] = torch.sigmoid(ze)[:, 0]
        d['out_eval'] = torch.sigmoid(ze) * y.double()
    return d


def _apply_fp32(t4, mean32, rstd32):
    """sa_gate_kernel: fp32 gamma * ((t - mean) * rstd) + beta, 1 / (1 + exp(-z))"""
    g, b = torch.tensor(GAMMA, dtype=torch.float32), torch.tensor(BETA, dtype=torch.float32)
    z = g * ((t4 - mean32) * rstd32) + b
    return (1.0 / (1.0 + torch.exp(-z)))[:, 0]


def gate_kernel_arithmetic(t4):
    """the arithmetic of bn1_stats_kernel + sa_gate_kernel: double sums, mean and rstd stored as fp32, fp32 apply -> gate"""
    a = t4.double().reshape(-1)
    m = a.numel()
    mean = a.sum() / m
    var = torch.clamp((a * a).sum() / m - mean * mean, min=0.0)
    return _apply_fp32(t4, mean.float(), (1.0 / torch.sqrt(var + float(np.float32(EPS)))).float())


def gate_naive_fp32(t4, lanes=1):
    """what the stats kernel must NOT be: fp32 running sums of x and x^2 (in element order; lanes > 1: one fp32 pair per thread of
    a `lanes`-thread block, element i on thread i % lanes, the partial sums then added exactly), var = E[x^2] - mean^2 -> gate"""
    a = t4.reshape(-1).numpy().astype(np.float32)
    m = a.size
    pad = (-m) % lanes
    a = np.concatenate([a, np.zeros(pad, np.float32)]).reshape(-1, lanes)
    s1 = np.cumsum(a, axis=0, dtype=np.float32)[-1].astype(np.float64).sum()
    s2 = np.cumsum(a * a, axis=0, dtype=np.float32)[-1].astype(np.float64).sum()
    if lanes == 1:
        mean = np.float32(np.float32(s1) / np.float32(m))
        var = np.float32(np.float32(s2) / np.float32(m)) - mean * mean
    else:
        mean = s1 / m
        var = s2 / m - mean * mean
    var = max(float(var), 0.0)
    return _apply_fp32(t4, torch.tensor(float(mean), dtype=torch.float32),
                       torch.tensor(1.0 / np.sqrt(var + float(np.float32(EPS))), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ transposed conv
@functools.lru_cache(maxsize=None)
def convt_case(n, ci, co, h, w):
    """-> dict: fp32 x [n,ci,h,w], w [ci,co,2,2], b [co], dy [n,co,2h,2w] and float64 y, y_nobias, dx, dw"""
    g = _gen(4, n, ci, co, h, w)
    d = dict(x=torch.randn(n, ci, h, w, generator=g), w=torch.randn(ci, co, 2, 2, generator=g) * (1.0 / ci ** 0.5),
             b=torch.randn(co, generator=g), dy=torch.randn(n, co, 2 * h, 2 * w, generator=g))
    xr, wr = d['x'].double().requires_grad_(True), d['w'].double().requires_grad_(True)
    y = F.conv_transpose2d(xr, wr, d['b'].double(), stride=2)
    y.backward(d['dy'].double())
    d['y'], d['dx'], d['dw'] = y.detach(), xr.grad, wr.grad
    d['y_nobias'] = d['y'] - d['b'].double().view(1, co, 1, 1)
    return d
