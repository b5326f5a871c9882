"""Cases, operands, references and error bounds of tests/test_gpu_bn_paths.py (training-mode BatchNorm2d + ReLU, csrc/bn.hip),
validated without a GPU by tests/test_bn_reference_host.py.  Plain torch / numpy; the references run on whatever device their
arguments live on (float64 throughout), so the GPU test evaluates them next to the kernel's outputs.

Path predictor: predict_fwd / predict_bwd / predict_apply restate coop_plan, pick_splits and the width rules of bn_train_fwd_t,
bn_relu_bwd_t and bn_relu_apply_t -> Plan(form, V, Q, S, per, splits); the GPU test pins them to the library (aide_bn_one_pass,
aide_bn_two_pass, aide_bn_relu_bwd_pool_supported, and the channel epochs a launch leaves in the workspace).

References
  1  ref_operator: float64 F.relu(F.batch_norm(z, training=True)) and its autograd, the statistics written out (mean, biased
     variance, rstd, running statistics with the unbiased variance).  A channel of ONE value takes the kernel's stated rule
     (var = 0, rstd = 1 / sqrt(eps), running_var moves towards the biased value): aten refuses that call.
  2  ref_contract: float64 evaluation of the kernel's contract under PRESCRIBED fp32 coefficients (mean, rstd, scale, shift):
     a = relu(z * scale + shift), mask = z * scale + shift > 0, xhat = (z - mean) * rstd, dbeta = sum dy, dgamma = sum dy xhat,
     dz = scale * (dy - fl(sum dy / n) - xhat * fl(sum dy xhat / n)), dbias = scale * ((sum dy - n c0) - c1 sum xhat).
     Its mask IS the kernel's mask: z * scale is exact in float64 (24 x 24 bits), the float64 sum with shift keeps the sign of
     the exact sum, and the kernel's fp32 fmaf rounds the same exact value once and cannot reach zero from a non-zero value
     of O(1) operands (test_bn_reference_host.py::test_mask_claim_exact proves it on the cases' values in rational arithmetic).

Bounds, per channel, u = 2^-24 (unit roundoff of fp32), e64 = (terms + 8) * 2^-53 (a float64 sum of `terms` values, any order);
every bound is multiplied by SLACK = 1 + 2^-20 for the products of two error terms it drops.  With A1 = mean |z|, A2 = mean z^2:
  dm    = e64 A1 + 2^-52 |mean|                 error of the float64 mean (sum, quotient) -- every form sums in float64 from the first value
  dvar  = e64 A2 + 2^-52 (A2 + mean^2) + 2 |mean| dm + dm^2          (sum of squares; quotient, square, difference in float64)
  r     = 1 / sqrt(1 - dvar / (var + eps)) - 1 + 2^-51               relative error of the float64 1 / sqrt(var + eps)
  mean  : u |mean| + dm                                              one rounding to fp32
  rstd  : rstd (u + r)                                               one rounding
  scale : |scale| (2 u + r)                                          + the product gamma * rstd
  shift : |mean scale| (4 u + r) + |scale| dm + u |shift|            mean (u), scale (2 u + r), the product (u); the difference (u)
  running_mean : u (|(1 - m) rm0| + 2 m |mean| + |new|) + m dm       (1 - m) * rm0, mean -> fp32, m * mean, the sum; m = 1/8 and
                                                                     1 - m are exact in fp32
  running_var  : u ((1 - m) rv0 + 2 m unb + new) + m dvar n / (n - 1)
  a     : u |y| + 2^-52 (|z scale| + |shift|)   against reference 2 under the DEVICE's coefficients: the fmaf's one rounding (and the
                                             reference's own float64 sum)
  backward, against reference 2 under the device's coefficients (no form keeps an fp32 partial sum: rule at the top of bn.hip):
  dS0   = e64 sum |dy|       dS1 = (2 u + e64) sum |dy xhat|       dS2 = (2 u + e64) sum |xhat|
                                             (2 u: the kernel's xhat = fl(fl(z - mean) * rstd) carries two roundings)
  dbeta : u |S0| + dS0              dgamma : u |S1| + dS1
  dc0   = dS0 / n + 2 u |c0|        dc1 = dS1 / n + 2 u |c1|            fl(x / n) of two nearby x: at most one fp32 spacing apart
  dz    : |scale| (u (|dy| + |c0|) + 3 u |xhat c1| + dc0 + |xhat| dc1 + u |T|) + u |scale T|,  T = dy - c0 - xhat c1
                                             uncontracted: fl(dy - c0), fl(xhat c1) on a twice-rounded xhat (3 u), the difference,
                                             the product with scale; the contracted form fma(-xhat, c1, fl(dy - c0)) has one rounding
                                             fewer and is covered
  dbias : |scale| (2 dS0 + 2 u |S0| + dc1 |S2| + |c1| dS2) + u |dbias|
A bf16-stored output is the fp32 value rounded to nearest even, and rounding is monotone: with the fp32 value inside [ref - b, ref + b]
the stored one lies inside [bf16(ref - b), bf16(ref + b)] (inside_bf16).  That is the sharpest statement the format allows; a relative
allowance would have to be 2^-8 |value| (8 significand bits: half a spacing just above a power of two), 2^-9 |value| refuses correctly
rounded values (measured: 1.99 of it on the (4, 640, 64, 64) row).
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from spatial_cases import GUARD, SENT, Layout  # noqa: F401  (re-exported to the two test files)

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
EPS = float(np.float32(1e-5))          # the kernel widens the fp32 eps it is given
MOM = 0.125                            # m and 1 - m exact in fp32
NBT0 = 3

# ------------------------------------------------------------------------------------------------ path predictor
BN_SLOTS = 256
WS_STRIDE = 8 + 4 * BN_SLOTS           # doubles per channel of the workspace
MAX_S = BN_SLOTS
MIN_WGS = 512
ONEPASS_MAX, ONEPASS_MAX_NARROW = 34 << 20, 9 << 20
Plan = collections.namedtuple('Plan', 'form V Q S per splits')


def coop_plan(n, c, hw, mod8, narrow=False):
    """-> (V, Q, S, per) of the one-pass form, or None"""
    v = 8 if (mod8 and hw % 8 == 0 and n * hw >= 2048) else 4
    if n * c * hw > (ONEPASS_MAX_NARROW if narrow else ONEPASS_MAX):
        return None
    if hw % v or n * hw // v > MAX_S * 256 * 8:
        return None
    units = n * hw // v

    def wgs(q):
        return (units + 256 * q - 1) // (256 * q)
    q = 32 // v
    s = wgs(q)
    while s > MAX_S and q < 8:
        q <<= 1
        s = wgs(q)
    if s > MAX_S:
        return None
    while q > 1 and c * s < MIN_WGS and s * 2 <= MAX_S:
        q >>= 1
        s = wgs(q)
    per = (units + s - 1) // s
    need = (per + 255) // 256
    return v, (1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8), s, per


def pick_splits(n, c, hw):
    total4 = n * hw // (4 if hw % 4 == 0 else 1)
    return max(1, min((2048 + c - 1) // c, (total4 + 255) // 256, 64))


def _two_pass(n, hw, v, splits):
    total = n * hw // v
    return Plan('two-pass', v, 0, 0, (total + splits - 1) // splits, splits)


def predict_fwd(shape, z_bs, a_bs, z_bf16=False, a_bf16=False, slabs=False, split_stride=0, groups=1):
    """bn_train_fwd_t; n = images PER GROUP.  form 'error': the launcher returns AIDE_ERR_ARG"""
    n, c, h, w = shape
    hw = h * w
    v4 = hw % 4 == 0 and z_bs % 4 == 0 and a_bs % 4 == 0
    if groups < 1 or (slabs and not v4):
        return Plan('error', 0, 0, 0, 0, 0)
    splits = pick_splits(n, c, hw)
    if groups > 1 and splits > 96 // groups:
        splits = max(96 // groups, 1)
    if groups * splits > 96:
        return Plan('error', 0, 0, 0, 0, 0)
    mod8 = z_bs % 8 == 0 and a_bs % 8 == 0 and (not slabs or split_stride % 8 == 0)
    cp = coop_plan(n, c, hw, mod8, z_bf16 or a_bf16) if v4 else None
    if cp:
        return Plan('one-pass', cp[0], cp[1], cp[2], cp[3], 0)
    v8 = v4 and not slabs and hw % 8 == 0 and z_bs % 8 == 0 and a_bs % 8 == 0
    return _two_pass(n, hw, 8 if v8 else 4 if v4 else 1, splits)


def predict_bwd(shape, d_bs, z_bs, dz_bs, d_bf16=False, z_bf16=False, dz_bf16=False):
    """bn_relu_bwd_t"""
    n, c, h, w = shape
    hw = h * w
    v4 = hw % 4 == 0 and z_bs % 4 == 0 and d_bs % 4 == 0 and dz_bs % 4 == 0
    mod8 = z_bs % 8 == 0 and d_bs % 8 == 0 and dz_bs % 8 == 0
    cp = coop_plan(n, c, hw, mod8, d_bf16 or z_bf16 or dz_bf16) if v4 else None
    if cp:
        return Plan('one-pass', cp[0], cp[1], cp[2], cp[3], 0)
    return _two_pass(n, hw, 8 if (v4 and hw % 8 == 0 and mod8) else 4 if v4 else 1, pick_splits(n, c, hw))


def predict_apply(shape, z_bs, a_bs):
    """unit width of bn_relu_apply_t"""
    hw = shape[2] * shape[3]
    return 4 if (hw % 4 == 0 and z_bs % 4 == 0 and a_bs % 4 == 0) else 1


def predict_parts(shape, z_bs, a_bs):
    """the conv-epilogue form: bn_train_apply_kernel<4> on given statistics, or an argument error"""
    n, c, h, w = shape
    ok = (h * w) % 4 == 0 and z_bs % 4 == 0 and a_bs % 4 == 0
    return Plan('parts', 4, 0, 0, 0, 0) if ok else Plan('error', 0, 0, 0, 0, 0)


def epoch_step(plan, groups=1):
    """what a launch adds to every channel's epoch: only a one-pass launch with S > 1 exchanges anything"""
    return groups if (plan.form == 'one-pass' and plan.S > 1) else 0


def one_pass(n, c, h, w):
    return 1 if coop_plan(n, c, h * w, True) else 0


def two_pass(n, c, h, w):
    return 0 if (n * h * w <= 256 * 16 * 4 and c >= 64) else 1


def pool_supported(n, c, h, w):
    cp = coop_plan(n, c, h * w, True)
    return 1 if (h % 2 == 0 and w % 8 == 0 and cp and cp[0] == 8) else 0


def batch_stride(kind, shape):
    return Layout(kind, shape).bs


def kinds_for(shape):
    """layout kinds whose view starts on a 16-byte boundary in fp32 and in bf16 ('hi' starts C*H*W elements in)"""
    chw = shape[1] * shape[2] * shape[3]
    return tuple(k for k in ('dense', 'lo', 'hi', 'pad1', 'pad2', 'pad4') if k != 'hi' or chw % 8 == 0)


# ------------------------------------------------------------------------------------------------ case tables
# kinds: layouts of (z, a, dA, dz).  fwd / bwd: the path the row is there for, (form, V, Q, S) -- for the two-pass form
# (form, V, 0, splits).  storage: bf16 flags of (z, a, dA, dz).
Row = collections.namedtuple('Row', 'name shape kinds fwd bwd storage big')
D4 = ('dense',) * 4
F4 = (False,) * 4


def _row(name, shape, path, kinds=D4, bwd=None, storage=F4, big=False):
    return Row(name, shape, kinds, path, bwd or path, storage, big)


ROWS = [
    _row('v4_s1', (2, 3, 4, 6), ('one-pass', 4, 1, 1)),                       # 12 units, 244 idle threads
    _row('v4_one_unit', (1, 1, 2, 2), ('one-pass', 4, 1, 1)),
    _row('v4_s2', (5, 8, 20, 20), ('one-pass', 4, 1, 2)),
    _row('v8_s2', (2, 6, 32, 40), ('one-pass', 8, 1, 2)),
    _row('v4_by_stride', (2, 6, 32, 40), ('one-pass', 4, 1, 3), kinds=('pad4',) * 4),   # ragged: 212 of 214 units in the last workgroup
    _row('v8_q1', (2, 600, 32, 32), ('one-pass', 8, 1, 1), big=True),
    _row('v8_q2', (3, 600, 36, 28), ('one-pass', 8, 2, 1), big=True),        # 378 units: ragged inside Q 2
    _row('v8_q4', (8, 600, 32, 32), ('one-pass', 8, 4, 1), big=True),
    _row('v8_q4_s2', (24, 260, 20, 20), ('one-pass', 8, 4, 2), big=True),
    _row('v8_q8', (16, 2, 512, 512), ('one-pass', 8, 8, 256), big=True),
    _row('v4_q8', (16, 2, 258, 258), ('one-pass', 4, 8, 131), big=True),
    _row('tp_v1_plane', (3, 5, 37, 41), ('two-pass', 1, 0, 18)),             # ragged per: 18 * 253 > 4551
    _row('tp_v1_tiny', (2, 4, 3, 2), ('two-pass', 1, 0, 1)),
    _row('tp_v1_pad1', (2, 6, 32, 40), ('two-pass', 1, 0, 3), kinds=('pad1',) * 4),
    _row('tp_v1_pad2', (2, 6, 32, 40), ('two-pass', 1, 0, 3), kinds=('pad2',) * 4),
    _row('tp_v1_one_value', (1, 3, 1, 1), ('two-pass', 1, 0, 1)),
    _row('tp_v4', (17, 1, 514, 514), ('two-pass', 4, 0, 64), big=True),
    _row('tp_v8', (17, 1, 512, 512), ('two-pass', 8, 0, 64), big=True),      # 557 056 units: over the per-channel limit
    _row('tp_v8_narrow', (4, 640, 64, 64), ('two-pass', 8, 0, 4), storage=(True,) * 4, big=True),     # over 9 Mi values
    _row('tp_v8_narrow_z', (4, 640, 64, 64), ('two-pass', 8, 0, 4), storage=(True, False, False, False), big=True),
]
ROW = {r.name: r for r in ROWS}
SMALL = [r.name for r in ROWS if not r.big]
# the instantiations the tables must reach (test_bn_reference_host.py::test_tables_reach_every_instantiation)
NEEDED = ([('one-pass', 4, q) for q in (1, 8)] + [('one-pass', 8, q) for q in (1, 2, 4, 8)] +
          [('two-pass', v, 0) for v in (1, 4, 8)])

# groups rows: (name, images per group, groups, C, H, W, kinds of (z, a), path)
GROUP_ROWS = [
    ('g3_v8', 2, 3, 6, 32, 40, ('dense', 'dense'), ('one-pass', 8, 1, 2)),
    ('g3_v4', 5, 3, 8, 20, 20, ('dense', 'dense'), ('one-pass', 4, 1, 2)),
    ('g3_tp_v1', 3, 3, 5, 37, 41, ('dense', 'dense'), ('two-pass', 1, 0, 18)),
    ('g13_tp_clamped', 8, 13, 2, 15, 15, ('dense', 'dense'), ('two-pass', 1, 0, 7)),    # pick_splits 8 -> 96 // 13 = 7
]
# stress rows: (name, shape, what)
STRESS = [(s, n, k) for s, n in (((5, 8, 20, 20), 'op'), ((3, 5, 37, 41), 'tp'))
          for k in ('constant', 'far_mean', 'no_gamma', 'no_beta', 'no_running', 'zero_preact')]
STORAGE_ROWS = ('v8_s2', 'v4_s2', 'tp_v1_plane', 'tp_v8_narrow')
FWD_STORAGE = [(z, a) for z in (False, True) for a in (False, True)]
BWD_STORAGE = [(d, z, o) for d in (False, True) for z in (False, True) for o in (False, True)]
PARTS_N = (1, 5, 64, 65, 130)
FINALIZE_GROUPS = (1, 3, 33, 40)


def row_plans(row):
    """-> (forward Plan, backward Plan, apply width) of a row as the predictor sees it"""
    bz, ba, bd, bo = (batch_stride(k, row.shape) for k in row.kinds)
    sz, sa, sd, so = row.storage
    return (predict_fwd(row.shape, bz, ba, sz, sa), predict_bwd(row.shape, bd, bz, bo, sd, sz, so),
            predict_apply(row.shape, bz, ba))


def path_of(plan):
    return (plan.form, plan.V, plan.Q, plan.S if plan.form == 'one-pass' else plan.splits)


def layout_sweep():
    """(shape, kinds of (z, a, dA, dz)) on the small shapes: every kind on all four tensors, and on (2, 6, 32, 40) each
    tensor alone on pad4 (V 8 -> 4) and on pad1 (-> the scalar two-pass kernels) -- one tensor's stride decides the width"""
    out = []
    for shape in ((2, 3, 4, 6), (5, 8, 20, 20), (2, 6, 32, 40), (3, 5, 37, 41)):
        out += [(shape, (k,) * 4) for k in kinds_for(shape) if k != 'dense']
    for k in ('pad4', 'pad1'):
        for i in range(4):
            out.append(((2, 6, 32, 40), tuple(k if j == i else 'dense' for j in range(4))))
    return out


# ------------------------------------------------------------------------------------------------ operands
def _clear_of_zero(z, y, scale, shift):
    """no pre-activation within 64 u of zero (in units of its own terms)"""
    return y.abs() > 64 * U * ((z.double() * scale).abs() + shift.abs() + 1.0)


def _coef64(z, gamma, beta):
    zd = z.double()
    mean, var = zd.mean((0, 2, 3)), zd.var((0, 2, 3), unbiased=False)
    scale = gamma.double() / torch.sqrt(var + EPS)
    return scale.view(1, -1, 1, 1), (beta.double() - mean * scale).view(1, -1, 1, 1)


@functools.lru_cache(maxsize=4)
def operands(shape, bf16=False, stress=None, seed=0):
    """-> dict(z, dA [N, C, H, W]; gamma, beta, rm0, rv0 [C]) fp32 on the CPU, seeded.  gamma in [0.5, 1.5] with channel 1
    negative and channel 2 exactly 0, beta of both signs and |beta| >= 0.05, running statistics away from (0, 1); dA of the last
    channel (C >= 4) is zero: c0 == c1 == 0 there.  bf16: z and dA hold bf16 values.  The values are moved until no
    pre-activation of the float64 operator lies within 64 u of zero (asserted), so that reference 2 under exact
    coefficients and reference 1 share one mask."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(7919 * seed + 131 * n + 17 * c + 3 * h + w)
    z = torch.randn(n, c, h, w, generator=g) * 1.7 + torch.randn(1, c, 1, 1, generator=g)
    dA = torch.randn(n, c, h, w, generator=g)
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.3
    beta = torch.where(beta < 0, beta.clamp(max=-0.05), beta.clamp(min=0.05))
    if c >= 2:
        gamma[1] = -gamma[1]
    if c >= 3:
        gamma[2] = 0.0
    if c >= 4:
        dA[:, c - 1] = 0.0
    if stress == 'constant':
        z[:, 0] = 0.75
    elif stress == 'far_mean':
        z[:, 0] = z[:, 0] / z[:, 0].std() + 1000.0          # |mean| / std = 1e3
    if bf16:
        z, dA = z.bfloat16().float(), dA.bfloat16().float()
    if n * h * w > 1:
        for _ in range(8):
            scale, shift = _coef64(z, gamma, beta)
            bad = ~_clear_of_zero(z, z.double() * scale + shift, scale, shift)
            if not bad.any():
                break
            z = torch.where(bad, z + 0.0625, z)
            if bf16:
                z = z.bfloat16().float()
        scale, shift = _coef64(z, gamma, beta)
        assert _clear_of_zero(z, z.double() * scale + shift, scale, shift).all()
    return dict(z=z, dA=dA, gamma=gamma, beta=beta, rm0=torch.randn(c, generator=g) * 0.5,
                rv0=torch.rand(c, generator=g) + 0.5)


def row_operands(row):
    return operands(row.shape, bf16=any(row.storage))


def stress_operands(shape, what):
    op = dict(operands(shape, stress=what if what in ('constant', 'far_mean') else None))
    if what == 'no_gamma':
        op['gamma'] = None
    elif what == 'no_beta':
        op['beta'] = None
    elif what == 'no_running':
        op['rm0'] = op['rv0'] = None
    elif what == 'zero_preact':                    # gamma = beta = 0 on channel 0: every pre-activation there is exactly 0, and 0 is masked off
        op['gamma'], op['beta'] = op['gamma'].clone(), op['beta'].clone()
        op['gamma'][0] = op['beta'][0] = 0.0
    return op


# ------------------------------------------------------------------------------------------------ reference 1
def channel_moments(z):
    """float64 (mean, biased var, mean |z|, mean z^2) per channel, on z's device"""
    zd = z.double()
    n = zd.shape[0] * zd.shape[2] * zd.shape[3]
    mean = zd.mean((0, 2, 3))
    var = zd.var((0, 2, 3), unbiased=False) if n > 1 else torch.zeros_like(mean)
    return mean, var, zd.abs().mean((0, 2, 3)), (zd * zd).mean((0, 2, 3))


def running_update(rm0, rv0, mean, var, n):
    unb = var * n / (n - 1) if n > 1 else var
    return (1 - MOM) * rm0.double() + MOM * mean, (1 - MOM) * rv0.double() + MOM * unb


def ref_operator(z, gamma, beta, rm0=None, rv0=None, dA=None, relu=True, stats_only=False):
    """reference 1 -> dict of float64: mean, var, rstd, scale, shift, A1, A2, (rm, rv), a, and with dA: dz, dgamma, dbeta"""
    n = z.shape[0] * z.shape[2] * z.shape[3]
    c = z.shape[1]
    mean, var, a1, a2 = channel_moments(z)
    g = gamma.double() if gamma is not None else torch.ones(c, dtype=torch.float64, device=z.device)
    b = beta.double() if beta is not None else torch.zeros(c, dtype=torch.float64, device=z.device)
    rstd = 1.0 / torch.sqrt(var + EPS)
    out = dict(mean=mean, var=var, rstd=rstd, scale=g * rstd, shift=b - mean * g * rstd, A1=a1, A2=a2, n=n)
    if rm0 is not None:
        out['rm'], out['rv'] = running_update(rm0, rv0, mean, var, n)
    if stats_only:
        return out
    if n == 1:                                     # aten refuses one value per channel: the kernel's stated rule
        y = z.double() * out['scale'].view(1, -1, 1, 1) + out['shift'].view(1, -1, 1, 1)
        out['a'] = torch.relu(y) if relu else y
        return out
    zr = z.double().clone().requires_grad_(dA is not None)
    gr, br = g.clone().requires_grad_(dA is not None), b.clone().requires_grad_(dA is not None)
    y = F.batch_norm(zr, None, None, gr, br, True, MOM, EPS)
    a = F.relu(y) if relu else y
    out['a'] = a.detach()
    if dA is not None:
        a.backward(dA.double())
        out['dz'], out['dgamma'], out['dbeta'] = zr.grad, gr.grad, br.grad
    return out


# ------------------------------------------------------------------------------------------------ reference 2
def _v(x):
    return x.double().view(1, -1, 1, 1)


def ref_forward(z, scale, shift, relu=True):
    """float64 (a, y) of the forward contract under given coefficients"""
    y = z.double() * _v(scale) + _v(shift)
    return (torch.relu(y) if relu else y), y


def ref_contract(z, dA, mean, rstd, scale, shift, relu=True):
    """reference 2 -> dict of float64 tensors (module docstring); the sums of magnitudes the bounds need ride along"""
    n = z.shape[0] * z.shape[2] * z.shape[3]
    a, y = ref_forward(z, scale, shift, relu)
    mask = (y > 0) if relu else torch.ones_like(y, dtype=torch.bool)
    xhat = (z.double() - _v(mean)) * _v(rstd)
    dy = torch.where(mask, dA.double(), torch.zeros_like(y))
    s0, s1, s2 = dy.sum((0, 2, 3)), (dy * xhat).sum((0, 2, 3)), xhat.sum((0, 2, 3))
    c0, c1 = (s0 / n).float().double(), (s1 / n).float().double()
    t = dy - _v(c0) - xhat * _v(c1)
    sc = scale.double()
    return dict(a=a, y=y, mask=mask, xhat=xhat, dy=dy, S0=s0, S1=s1, S2=s2, c0=c0, c1=c1, T=t, dz=_v(sc) * t,
                dbeta=s0, dgamma=s1, dbias=sc * ((s0 - n * c0) - c1 * s2), n=n,
                abs_dy=dy.abs().sum((0, 2, 3)), abs_dyx=(dy * xhat).abs().sum((0, 2, 3)), abs_x=xhat.abs().sum((0, 2, 3)))


# ------------------------------------------------------------------------------------------------ bounds
def e64(terms):
    return (terms + 8) * 2.0 ** -53


def stat_bounds(r1, gamma, beta, rm0, rv0, terms=None, mean_pre=None, dm_extra=0.0, dvar_extra=0.0):
    """bounds of mean, rstd, scale, shift, rm, rv against a reference dict r1 (ref_operator's keys).  terms: number of float64 summands (default n); mean_pre: the mean that enters E[x^2] - mean^2 when it is
    not the final one (conv-epilogue statistics: the sums are of z - bias); *_extra: rounding the inputs already carry."""
    n = r1['n']
    mean, var, rstd, scale, shift = (r1[k] for k in ('mean', 'var', 'rstd', 'scale', 'shift'))
    e = e64(n if terms is None else terms)
    mp = mean if mean_pre is None else mean_pre
    dm = e * r1['A1'] + dm_extra + 2.0 ** -52 * mean.abs()
    dvar = e * r1['A2'] + 2.0 ** -52 * (r1['A2'] + mp * mp) + 2 * mp.abs() * dm + dm * dm + dvar_extra
    ratio = dvar / (var + EPS)
    assert float(ratio.max()) < 0.5, 'the variance is not determined to within half of itself'
    r = 1.0 / torch.sqrt(1.0 - ratio) - 1.0 + 2.0 ** -51
    out = dict(mean=U * mean.abs() + dm, rstd=rstd * (U + r), scale=scale.abs() * (2 * U + r),
               shift=(mean * scale).abs() * (4 * U + r) + scale.abs() * dm + U * shift.abs())
    if rm0 is not None:
        unb = var * n / (n - 1) if n > 1 else var
        out['rm'] = U * (((1 - MOM) * rm0.double()).abs() + 2 * MOM * mean.abs() + r1['rm'].abs()) + MOM * dm
        out['rv'] = U * ((1 - MOM) * rv0.double().abs() + 2 * MOM * unb + r1['rv'].abs()) + MOM * dvar * (n / (n - 1) if n > 1 else 1.0)
    return {k: v * SLACK for k, v in out.items()}


def a_bound(z, y, scale, shift):
    return (U * y.abs() + 2.0 ** -52 * ((z.double() * _v(scale)).abs() + _v(shift).abs())) * SLACK


def bwd_bounds(r2, scale):
    """bounds of dz (elementwise), dgamma, dbeta, dbias against ref_contract's dict"""
    n = r2['n']
    e = e64(n)
    ds0 = e * r2['abs_dy']
    ds1 = (2 * U + e) * r2['abs_dyx']
    ds2 = (2 * U + e) * r2['abs_x']
    c0, c1, sc = r2['c0'], r2['c1'], scale.double().abs()
    dc0, dc1 = ds0 / n + 2 * U * c0.abs(), ds1 / n + 2 * U * c1.abs()
    xa = r2['xhat'].abs()
    dz = _v(sc) * (U * (r2['dy'].abs() + _v(c0.abs())) + 3 * U * xa * _v(c1.abs()) + _v(dc0) + xa * _v(dc1) + U * r2['T'].abs()) \
        + U * r2['dz'].abs()
    out = dict(dz=dz, dbeta=U * r2['S0'].abs() + ds0, dgamma=U * r2['S1'].abs() + ds1,
               dbias=sc * (2 * ds0 + 2 * U * r2['S0'].abs() + dc1 * r2['S2'].abs() + c1.abs() * ds2) + U * r2['dbias'].abs())
    return {k: v * SLACK for k, v in out.items()}


def inside_bf16(got, ref, bound):
    """a bf16-stored output whose fp32 value lies within `bound` of `ref`: inside [bf16(ref - bound), bf16(ref + bound)] (the rounding
    to fp32 and the rounding to nearest even bf16 are both monotone)"""
    lo, hi = (ref.double() - bound).float().bfloat16().float(), (ref.double() + bound).float().bfloat16().float()
    g = got.float()
    return bool(((g >= lo) & (g <= hi)).all())


def share(got, ref, bound):
    """largest |got - ref| / bound; a zero bound admits only equality"""
    err = (got.double() - ref.double()).abs()
    b = bound if isinstance(bound, torch.Tensor) else torch.full_like(err, bound)
    s = torch.where(b > 0, err / b.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(s.max()) if s.numel() else 0.0


# ------------------------------------------------------------------------------------------------ fp32 emulation (host)
def _f32(x):
    return x.float().double()


def emulate(z, dA, gamma, beta, rm0, rv0, relu=True):
    """A plain fp32 evaluation of the kernels' arithmetic on the CPU (one arithmetic for every form: float64 sums of the values, every
    coefficient operation rounded to fp32, the fmaf as one rounding of the float64 value, dz uncontracted) -> dict with the
    kernel's outputs."""
    n_, c, h, w = z.shape
    n = n_ * h * w
    zd = z.double()
    mean = zd.sum((0, 2, 3)) / n
    var = ((zd * zd).sum((0, 2, 3)) / n - mean * mean).clamp(min=0.0)
    rstd = _f32(1.0 / torch.sqrt(var + EPS))
    g = gamma.double() if gamma is not None else torch.ones(c, dtype=torch.float64)
    b = beta.double() if beta is not None else torch.zeros(c, dtype=torch.float64)
    sc = _f32(g * rstd)
    sh = _f32(b - _f32(_f32(mean) * sc))
    out = dict(mean=_f32(mean), rstd=rstd, scale=sc, shift=sh)
    if rm0 is not None:
        unb = var * n / (n - 1) if n > 1 else var
        out['rm'] = _f32(_f32((1 - MOM) * rm0.double()) + _f32(MOM * _f32(mean)))
        out['rv'] = _f32(_f32((1 - MOM) * rv0.double()) + _f32(MOM * _f32(unb)))
    y = _f32(zd * _v(sc) + _v(sh))
    out['a'] = torch.relu(y) if relu else y
    on = (y > 0) if relu else torch.ones_like(y, dtype=torch.bool)
    dy = torch.where(on, dA.double(), torch.zeros_like(y))
    xh = _f32(_f32(zd - _v(out['mean'])) * _v(rstd))
    s0, s1, s2 = dy.sum((0, 2, 3)), (dy * xh).sum((0, 2, 3)), xh.sum((0, 2, 3))
    c0, c1 = _f32(s0 / n), _f32(s1 / n)
    out['dz'] = _f32(_v(sc) * _f32(_f32(dy - _v(c0)) - _f32(xh * _v(c1))))
    out['dbeta'], out['dgamma'] = _f32(s0), _f32(s1)
    out['dbias'] = _f32(sc * ((s0 - n * c0) - c1 * s2))
    return out


# ------------------------------------------------------------------------------------------------ conv-epilogue statistics
def make_parts(z, conv_bias, nparts, groups=1, stride=None):
    """the statistics a convolution's epilogue would leave: every channel of z - conv_bias (per group of the stacked batch) cut into
    nparts contiguous pieces, fp32 sum and sum of squares each (one rounding of the float64 sum) -> parts [C, stride, 2] fp32, NaN in
    the entries no group owns"""
    nt, c, h, w = z.shape
    m = nt // groups
    stride = nparts * groups if stride is None else stride
    parts = torch.full((c, stride, 2), float('nan'), dtype=torch.float32, device=z.device)
    x = z.double() - (_v(conv_bias) if conv_bias is not None else 0.0)
    for gi in range(groups):
        flat = x[gi * m:(gi + 1) * m].permute(1, 0, 2, 3).reshape(c, -1)
        for i, piece in enumerate(torch.tensor_split(flat, nparts, dim=1)):
            parts[:, gi * nparts + i, 0] = piece.sum(1).float()
            parts[:, gi * nparts + i, 1] = (piece * piece).sum(1).float()
    return parts


def ref_from_parts(parts, first, nparts, n, conv_bias, gamma, beta):
    """reference of the parts form: the fp32 entries [first, first + nparts) summed in float64 -> ref_operator-style dict (A1, A2: the
    magnitudes the bounds take, from the entries themselves; P1 = sum |entry sums| / n: what one rounding per entry can move the mean by, in u)"""
    p = parts[:, first:first + nparts].double()
    s, ss = p[..., 0].sum(1), p[..., 1].sum(1)
    c = parts.shape[0]
    mean_pre = s / n
    var = (ss / n - mean_pre * mean_pre).clamp(min=0.0)
    mean = mean_pre + (conv_bias.double() if conv_bias is not None else 0.0)
    g = gamma.double() if gamma is not None else torch.ones(c, dtype=torch.float64, device=parts.device)
    b = beta.double() if beta is not None else torch.zeros(c, dtype=torch.float64, device=parts.device)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return dict(mean=mean, mean_pre=mean_pre, var=var, rstd=rstd, scale=g * rstd, shift=b - mean * g * rstd, n=n,
                A1=p[..., 0].abs().sum(1) / n + mean.abs(), A2=ss / n, P1=p[..., 0].abs().sum(1) / n)


def eval_fold_ref(gamma, beta, rm, rv, conv_bias):
    """float64 (scale, shift, fbias) of the eval-mode fold, and their bounds: rstd = 1.0f / sqrtf(rv + eps): the sum (u, halved by the
    root), sqrtf and the quotient to within one fp32 spacing each (2 u) -> 4.5 u; scale = g * rstd (+ u); shift = b - rm * scale
    (product, difference); fbias = fmaf(cb, scale, shift)"""
    c = rm.numel()
    g = gamma.double() if gamma is not None else torch.ones(c, dtype=torch.float64, device=rm.device)
    b = beta.double() if beta is not None else torch.zeros(c, dtype=torch.float64, device=rm.device)
    cb = conv_bias.double() if conv_bias is not None else torch.zeros(c, dtype=torch.float64, device=rm.device)
    scale = g / torch.sqrt(rv.double() + EPS)
    shift = b - rm.double() * scale
    fbias = cb * scale + shift
    bs = 5.5 * U * scale.abs()
    bsh = (rm.double() * scale).abs() * 6.5 * U + U * shift.abs()
    bf = cb.abs() * bs + bsh + U * fbias.abs()
    return (scale, shift, fbias), tuple(x * SLACK for x in (bs, bsh, bf))
